"""The encoder's overlaid sub-histogram (EncSmem::hist_view, L <= 11, one
block per wave) against the oracle, on the smallest inputs where the overlay
can go wrong: the view runs over the first 2,176 bytes of the phase-1 scratch
(the header words / spread symbols and the front of `norm`), so every block
here must give the oracle's bytes, length, payload bits, status and sidecar,
in both formats, through the blocks and the streams entry points -- and the
same at 10 and at 12 resident workgroups per CU (the diagnostics build's
FSEHIP_ENC_WGS), where a workgroup's LDS neighbours differ."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

CKPT = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _inputs():
    """{name: (block_size, [blocks])}: every block but the last of a batch has block_size bytes."""
    rng = np.random.default_rng(0x0E71A7)

    def g(p, seed, n):
        return O.generate(0, p, seed, 0, n)

    a4k, b4k = g(0.155, 0xE101, 4096), g(0.4, 0xE102, 4096)
    short = {2: np.array([7, 200], np.uint8), 3: np.array([1, 2, 1], np.uint8), 17: g(0.3, 0xE103, 17),
             4095: g(0.155, 0xE104, 4095), 4096: g(0.6, 0xE105, 4096)}
    # all 256 symbols: the view is written to its last bin and `norm` is used to its last entry
    full4k = rng.permutation(np.arange(4096) % 256).astype(np.uint8)
    full64k = rng.integers(0, 256, 65536, dtype=np.uint8)
    assert len(np.unique(full4k)) == 256 and len(np.unique(full64k)) == 256
    # skewed blocks that take the hot-symbol path (at least half of the first 1 KiB is the
    # first byte): the hot symbol's 32 words are the last bytes of the view
    skew = g(0.77, 0xE106, 65536)
    skew_hi = skew ^ np.uint8(0xC9)  # the same with symbol 201 hot and a 256-entry table
    for s in (skew, skew_hi):
        assert int((s[:1024] == s[0]).sum()) >= 512
    c2 = g(0.155, 0xE107, 65536)
    cases = {}
    for n, x in short.items():
        cases[f"one_{n}"] = (4096, [x])
        if n != 4096:
            cases[f"three_{n}"] = (4096, [a4k, b4k, x])
    cases["two_4096"] = (4096, [a4k, short[4096]])
    cases["full_4096"] = (4096, [full4k, a4k, full4k[::-1].copy()])
    cases["one_65536"] = (65536, [c2])
    cases["three_65536"] = (65536, [full64k, skew, c2])
    cases["two_65536"] = (65536, [skew_hi, full64k[::-1].copy()])
    cases["len_1"] = (4096, [np.array([5], np.uint8)])  # TOO_SHORT
    # blocks longer than a histogram segment (2^18 bytes): the view is zeroed again between
    # the segments; three segments of a skewed block, then two of a ragged one
    cases["segments"] = (2**19, [g(0.77, 0xE108, 2**19), g(0.155, 0xE109, 2**18 + 4096)])
    streams = [g(0.155, 0xE10A, 70001), full4k, np.array([3, 9], np.uint8), np.zeros(0, np.uint8),
               np.array([5], np.uint8), skew_hi[:40001], g(0.5, 0xE10B, 4095)]
    return cases, streams


def _want(x, nstates):
    """The oracle's (bytes, payload bits, sidecar words) of one block, or its status name."""
    try:
        comp, bits = (O.compress2 if nstates == 2 else O.compress)(x)
    except O.OracleError as e:
        return e.code
    if nstates == 2:
        bp, s0, s1 = O.checkpoints2(comp, CKPT)
        side = bp.astype(np.uint64) | (s0.astype(np.uint64) << 32) | (s1.astype(np.uint64) << 48)
    else:
        bp, s0 = O.checkpoints1(comp, CKPT)
        side = bp.astype(np.uint64) | (s0.astype(np.uint64) << 32)
    return comp, bits, side


_REF = {}


def reference():
    """Inputs and the oracle's results, computed once per process."""
    if not _REF:
        cases, streams = _inputs()
        _REF["cases"], _REF["streams"] = cases, streams
        for ns in (2, 1):
            _REF[ns] = ({k: [_want(x, ns) for x in blocks] for k, (_, blocks) in cases.items()},
                        [_want(x, ns) for x in streams])
    return _REF


def check_all(torch):
    """Every case through fsehip_compress_blocks and fsehip_compress_streams in both formats,
    equal to the oracle; returns a digest of everything the library produced."""
    from entropy_coders_amd import BlockCodec, compress_streams
    from entropy_coders_amd._lib import STATUS

    ref = reference()
    h = hashlib.sha256()
    for ns in (2, 1):
        want_blocks, want_streams = ref[ns]
        for name, (bs, blocks) in ref["cases"].items():
            codec = BlockCodec(block_size=bs, ckpt_interval=CKPT, nstates=ns)
            cb = codec.compress(torch.from_numpy(np.concatenate(blocks)).cuda())
            torch.cuda.synchronize()
            st = cb["status"].cpu().numpy()
            lens = cb["comp_len"].cpu().numpy()
            bits = cb["payload_bits"].cpu().numpy()
            side = cb["sidecar"].cpu().numpy().view(np.uint64)
            assert len(st) == len(blocks), (ns, name)
            for b, w in enumerate(want_blocks[name]):
                tag = (ns, name, b)
                if isinstance(w, str):
                    assert STATUS.get(int(st[b])) == w, tag
                    assert lens[b] == 0, tag
                    h.update(w.encode())
                    continue
                comp, wbits, wside = w
                got = codec.block_bytes(cb, b)
                assert st[b] == 0, tag + (int(st[b]),)
                assert lens[b] == len(comp), tag
                assert got == comp, tag
                assert int(bits[b]) & 0xFFFFFFFF == wbits, tag
                mine = side[b * codec.side_per_block: b * codec.side_per_block + len(wside)]
                assert np.array_equal(mine, wside), tag
                h.update(got + mine.tobytes() + bytes([int(bits[b]) & 0xFF]))
        got = compress_streams(ref["streams"], nstates=ns)
        assert len(got) == len(want_streams)
        for i, (gs, w) in enumerate(zip(got, want_streams)):
            if isinstance(w, str):
                assert gs == w, (ns, "stream", i, gs)
                h.update(w.encode())
            else:
                assert not isinstance(gs, str), (ns, "stream", i, gs)
                assert gs[0] == w[0] and gs[1] == w[1], (ns, "stream", i)
                h.update(gs[0])
    return h.hexdigest()


def test_overlay_exact(torch_cuda):
    assert len(check_all(torch_cuda)) == 64


_CHILD = """
import os, torch
import entropy_coders_amd._lib as L
import tests.test_gpu_enc_overlay as t
assert L.LIB_PATH.endswith('libfsehip_diag.so')
for wgs in ('10', '12'):
    os.environ['FSEHIP_ENC_WGS'] = wgs
    print('digest', wgs, t.check_all(torch))
print('child-ok')
"""


def test_overlay_exact_at_10_and_12_per_cu(torch_cuda):
    """The same at 10 and at 12 workgroups per CU, chosen by whole LDS granules in a child
    process on the diagnostics build (the product library reads no environment): equal to
    the oracle there too, so the bytes are identical to the product's."""
    if not os.path.exists(os.path.join(ROOT, "entropy_coders_amd", "libfsehip_diag.so")):
        pytest.fail("libfsehip_diag.so missing: build it (make -C entropy_coders_amd diag / __graft_entry__.build())")
    mine = check_all(torch_cuda)
    env = dict(os.environ, FSEHIP_LIB="libfsehip_diag.so", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child-ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    digests = [ln.split()[2] for ln in r.stdout.splitlines() if ln.startswith("digest")]
    assert digests == [mine, mine], (mine, digests)
