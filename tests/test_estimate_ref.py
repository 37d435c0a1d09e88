"""The size estimate's model against the CPU reference (no GPU, no library
under test): tests/estimate_ref.py beside frame_ref / planes_ref / delta_ref
and the oracle's block coder.  The reference is deterministic, so the caps
below document the model (DESIGN.md section 5 "Estimate" holds the measured
values); they cannot flake."""
import math
import os

import numpy as np
import pytest

import estimate_ref as E
import frame_ref as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, CKPT, NSTATES = 65536, 64, 2


def test_log2q8_every_count():
    worst = 0.0
    for c in range(1, 32769):
        worst = max(worst, abs(E.log2q8(c) - 256.0 * math.log2(c)))
    print(f"\n[estimate] log2q8: worst |y - 256 log2 c| = {worst:.4f}")
    assert worst <= 1.01
    for k in range(16):
        assert E.log2q8(1 << k) == 256 * k
    assert E.cost8(-1, 11) == E.cost8(1, 11) == 256 * 11 and E.cost8(1 << 11, 11) == 0


@pytest.fixture(scope="module")
def six():
    """name -> (estimates, real lengths) of the six tensors at 2^18 elements."""
    out = {}
    for name, a in E.six_tensors().items():
        out[name] = (E.container_estimates(a, BLOCK, nstates=NSTATES, ckpt=CKPT),
                     E.real_lengths(a, BLOCK, CKPT, NSTATES))
    return out


def test_six_tensors_lengths(six):
    worst = 0.0
    for name, (est, real) in six.items():
        for kind in E.KINDS:
            off = abs(est[kind] - real[kind]) / real[kind]
            worst = max(worst, off)
            print(f"[estimate] {name:20s} {E.NAMES[kind]:6s} est {est[kind]:8d} real {real[kind]:8d} {100 * off:.3f} %")
            assert off <= 0.02, (name, kind, est[kind], real[kind])
    print(f"[estimate] worst {100 * worst:.3f} %")


def test_six_tensors_choice(six):
    chosen = []
    for name, (est, real) in six.items():
        want = min(E.KINDS, key=lambda k: (real[k], k))
        assert E.choose(est) == want, (name, est, real)
        chosen.append(E.NAMES[want])
    assert chosen == ["delta", "delta", "delta", "delta", "planes", "planes"]


def test_choose_ties_and_none():
    N = E.NONE
    assert E.choose([5, 5, 5]) == E.FRAME and E.choose([6, 5, 5]) == E.PLANES and E.choose([6, 6, 5]) == E.DELTA
    assert E.choose([N, 7, 7]) == E.PLANES and E.choose([N, N, 0]) == E.DELTA and E.choose([N, N, N]) == -1
    assert E.choose({0: 9, 1: N, 2: 9}) == E.FRAME


def text_blocks():
    """Three 64 KiB blocks of English and tables: DESIGN.md's own first 192 KiB."""
    data = np.frombuffer(open(os.path.join(ROOT, "DESIGN.md"), "rb").read(), dtype=np.uint8)
    assert data.size >= 3 * BLOCK
    return [("text%d" % b, data[b * BLOCK:(b + 1) * BLOCK]) for b in range(3)]


def lut_blocks():
    return [(f"lut p={p} n={n}", O.generate(0, p, 1, 0, n)) for p in (0.05, 0.155, 0.5, 0.77) for n in (4096, 65536)]


@pytest.mark.parametrize("nstates", [2, 1])
def test_block_comp_length(nstates):
    worst = {4096: 0.0, 65536: 0.0}
    for name, blk in text_blocks() + lut_blocks():
        n = blk.size
        counts = np.bincount(blk, minlength=256)
        typ, rec, bits, L = E.block_estimate(counts, n, nstates=nstates, ckpt=0)
        _, comp = R.encode_block(blk, nstates, 0)
        assert typ == R.FSE, name
        off = (rec - len(comp)) / len(comp)
        worst[n] = max(worst[n], abs(off))
        print(f"[estimate] {name:22s} {nstates}-state est {rec:6d} real {len(comp):6d} {100 * off:+.3f} %")
        assert abs(off) <= (0.005 if n == 65536 else 0.01), (name, rec, len(comp))
    print(f"[estimate] {nstates}-state worst: 64 KiB {100 * worst[65536]:.3f} %, 4 KiB {100 * worst[4096]:.3f} %")


@pytest.mark.parametrize("nstates", [2, 1])
@pytest.mark.parametrize("tail", [1000, 1])
def test_block_types_on_the_corpus(nstates, tail):
    raw = R.corpus(tail)
    frame = R.build_frame(raw, R.BLOCK, R.CKPT, nstates)
    _, directory, _ = R.split_frame(frame)
    counts = E.counts_of(raw, R.BLOCK)
    est = E.block_estimates(counts, raw.size, R.BLOCK, nstates=nstates, ckpt=R.CKPT)
    left_out = 0
    for b, ((typ, stored), e) in enumerate(zip(directory, est)):
        n = R.raw_len(raw.size, R.BLOCK, b)
        if typ == R.FSE:
            real_rec = stored + 8 * R.spb_of(n, R.CKPT, nstates)
        elif typ == R.RAW:  # what the FSE record would have taken, when the coder ran at all
            status, comp = R.encode_block(raw[b * R.BLOCK:b * R.BLOCK + n], nstates, 0)
            real_rec = len(comp) + 8 * R.spb_of(n, R.CKPT, nstates) if status == "OK" else None
        else:
            real_rec = None
        if real_rec is not None and abs(real_rec - n) <= 0.01 * n:
            left_out += 1
            continue
        assert e[0] == typ, (b, e, typ, stored)
    assert left_out * 10 <= len(directory), left_out
