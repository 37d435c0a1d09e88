"""The size estimate (include/fsehip.h section 2g) restated in Python integers
over the CPU oracle and tests/frame_ref.py, planes_ref.py and delta_ref.py: a
helper for the estimate tests, not a test.

  log2q8, cost8        the fixed-point log and the cost of one symbol
  block_estimate       byte counts of one block -> (type, rec, bits, table log)
  image_counts         raw bytes -> the 256-bin counts of every block of a kind's image
  frame_estimate       per-block counts -> the frame's estimated length
  container_estimates  an array -> the three containers' estimated lengths
  choose               the smallest, ties to frame, then planes, then delta
  six_tensors          the tensors DESIGN.md section 5 "Estimate" is measured on

Nothing here calls the library under test.
"""
import numpy as np

import delta_ref as DR
import frame_ref as R
import planes_ref as PR
from oracle import oracle as O

FRAME, PLANES, DELTA = 0, 1, 2
KINDS = (FRAME, PLANES, DELTA)
NAMES = {FRAME: "frame", PLANES: "planes", DELTA: "delta"}
NONE = (1 << 64) - 1  # a kind that was not asked for, or whose width it does not take


def log2q8(c):
    """256 * log2(c) for 1 <= c <= 32768, within 1.01: the integer part, then
    eight squarings of the mantissa (31 fraction bits), one bit each."""
    assert 1 <= c <= 32768
    hb = c.bit_length() - 1
    x = c << (31 - hb)
    y = hb
    for _ in range(8):
        x = (x * x) >> 31
        y <<= 1
        if x >> 32:
            x >>= 1
            y |= 1
    return y


def cost8(c, L):
    """Bits * 256 of one symbol whose normalised count is c (-1 counts as 1)."""
    return 256 * L - log2q8(max(c, 1))


def hist_of(counts, raw_len):
    h = O.Hist()
    tl = 1
    for s in range(256):
        h.counts[s] = int(counts[s])
        if counts[s]:
            tl = s + 1
    h.size = raw_len
    h.table_len = tl
    return h


def block_estimate(counts, raw_len, nstates=2, ckpt=0, table_log=0, max_table_log=None):
    """(type, rec, bits, log) of a block from its byte counts: rec the
    record's estimated bytes (checkpoints included), bits the estimated
    payload bits and log the table log of an FSE block, 0 and 0 otherwise."""
    counts = [int(c) for c in counts]
    assert sum(counts) == raw_len
    if raw_len and counts[0] == raw_len:
        return R.RLE, 1, 0, 0
    h = hist_of(counts, raw_len)
    try:
        if raw_len == 0:
            raise O.OracleError(-1)
        L = O.optimal_log2(h) if table_log == 0 else table_log
        nh, _ = O.normalize(h, L)
        if raw_len < 2:
            raise O.OracleError(-2)
        hdr = len(O.header_write(nh))
    except O.OracleError:  # TOO_SHORT, CURSED: whatever the encoder's statistics refuse
        return R.RAW, raw_len, 0, 0
    L = nh.log2
    if L > (R.kernel_class(table_log) if max_table_log is None else max_table_log):
        return R.RAW, raw_len, 0, 0
    q = sum(counts[s] * cost8(nh.norm[s], L) for s in range(256) if counts[s])
    bits = ((q + 255) >> 8) + nstates * L + 1
    rec = hdr + (bits + 7) // 8 + 8 * R.spb_of(raw_len, ckpt, nstates)
    if rec < raw_len:
        return R.FSE, rec, bits, L
    return R.RAW, raw_len, 0, 0


def kind_image(raw, w, kind):
    """The bytes a kind's inner frame codes: the raw bytes, the plane image or
    the delta image."""
    raw = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8))
    if kind == FRAME:
        return raw
    if kind == PLANES:
        assert w in (2, 4, 8)
        return PR.image(raw, w)
    return DR.image(raw, w)


def counts_of(img, block_size):
    """uint32 [n_blocks, 256]: np.bincount of every block."""
    img = np.asarray(img, dtype=np.uint8)
    nb = R.n_blocks_of(img.size, block_size)
    key = np.arange(img.size, dtype=np.int64) // block_size * 256 + img
    return np.bincount(key, minlength=nb * 256).astype(np.uint32).reshape(nb, 256)


def image_counts(raw, w, kind, block_size):
    return counts_of(kind_image(raw, w, kind), block_size)


def block_estimates(counts, n_image, block_size, **kw):
    """block_estimate of every row of image_counts."""
    return [block_estimate(row, R.raw_len(n_image, block_size, b), **kw) for b, row in enumerate(counts)]


def frame_estimate(counts, n_image, block_size, **kw):
    return 32 + 4 * len(counts) + sum(e[1] for e in block_estimates(counts, n_image, block_size, **kw))


def container_estimates(a, block_size, kinds=KINDS, **kw):
    """{kind: estimated container bytes} of an array; NONE where the kind is
    not in `kinds` or does not take the element width."""
    a = np.ascontiguousarray(a).reshape(-1)
    w, raw = a.dtype.itemsize, PR.raw_bytes(a)
    out = {}
    for kind in KINDS:
        if kind not in kinds or (kind == PLANES and w == 1) or w not in (1, 2, 4, 8):
            out[kind] = NONE
            continue
        img = kind_image(raw, w, kind)
        inner = frame_estimate(counts_of(img, block_size), img.size, block_size, **kw)
        out[kind] = (0 if kind == FRAME else 16) + inner
    return out


def choose(est):
    """The kind of the smallest estimate (a dict or a 3-sequence), ties to
    the lower kind; -1 when every entry is NONE."""
    best = -1
    for kind in KINDS:
        if est[kind] != NONE and (best < 0 or est[kind] < est[best]):
            best = kind
    return best


def real_lengths(a, block_size, ckpt, nstates, table_log=0):
    """{kind: len of the reference container} of an array."""
    a = np.ascontiguousarray(a).reshape(-1)
    out = {FRAME: len(R.build_frame(PR.raw_bytes(a), block_size, ckpt, nstates, table_log)),
           DELTA: len(DR.build(a, block_size, ckpt, nstates, table_log))}
    if a.dtype.itemsize > 1:
        out[PLANES] = len(PR.build(a, block_size, ckpt, nstates, table_log))
    return out


def bf16_weights(n=1 << 18, seed=7):
    """standard_normal * 0.02 truncated to bf16, as uint16."""
    x = (np.random.default_rng(seed).standard_normal(n) * 0.02).astype(np.float32)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def six_tensors(n=1 << 18):
    """delta_ref.table_rows(n, 1) and the bf16 weights: name -> array."""
    rows = dict(DR.table_rows(n, 1))
    rows["bf16 weights"] = bf16_weights(n)
    return rows
