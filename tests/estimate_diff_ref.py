"""The size estimate with a base (include/fsehip.h section 2i) restated over
tests/estimate_ref.py and tests/diff_ref.py: a helper for the estimate-diff
tests, not a test.

  diff_counts   raw bytes of x and of the base -> the 256-bin counts of every block of the diff image
  estimates5    two arrays -> the five entries of fsehip_estimate_base
  choose5       the smallest; ties to frame, then planes, then delta, then diff
  real5         the reference containers' lengths, the diff frame's among them

Nothing here calls the library under test.
"""
import numpy as np

import diff_ref as D
import estimate_ref as E

FRAME, PLANES, DELTA, SEALED, DIFF = 0, 1, 2, 3, 4
NONE = E.NONE
NAMES = {FRAME: "frame", PLANES: "planes", DELTA: "delta", DIFF: "diff"}
ORDER = (FRAME, PLANES, DELTA, DIFF)  # the tie rule: a container that needs its base wins only when strictly smaller


def diff_counts(raw, base_raw, w, bs):
    """uint32 [n_blocks, 256] of the diff image of the raw element bytes."""
    return E.counts_of(D.image(raw, base_raw, w), bs)


def diff_estimate(a, b, bs, **kw):
    """16 + the frame estimate of the diff image of array a against b."""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    w = a.dtype.itemsize
    assert b.dtype.itemsize == w and a.size == b.size
    img = D.image(D.raw_bytes(a), D.raw_bytes(b), w)
    return 16 + E.frame_estimate(E.counts_of(img, bs), img.size, bs, **kw)


def estimates5(a, b, bs, kinds=ORDER, **kw):
    """[est of kind 0..4] as fsehip_estimate_base gives them: entry 3 always
    NONE, a kind not in `kinds` or not taking the width NONE."""
    three = E.container_estimates(a, bs, kinds=tuple(k for k in kinds if k in E.KINDS), **kw)
    return [three[FRAME], three[PLANES], three[DELTA], NONE, diff_estimate(a, b, bs, **kw) if DIFF in kinds else NONE]


def choose5(est):
    """The kind of the smallest of est[0], est[1], est[2], est[4] that is not
    NONE, the earliest of ORDER among equals; -1 when none is left."""
    best = -1
    for kind in ORDER:
        if est[kind] != NONE and (best < 0 or est[kind] < est[best]):
            best = kind
    return best


def real5(a, b, bs, ckpt, nstates, table_log=0):
    """{kind: len of the reference container}, kinds that take the width."""
    out = E.real_lengths(a, bs, ckpt, nstates, table_log)
    out[DIFF] = len(D.build(a, b, bs, ckpt, nstates, table_log))
    return out
