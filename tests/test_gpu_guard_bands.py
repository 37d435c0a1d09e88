"""Where the batched device entry points write: every output array sits
between two guard bands, so a store past a ragged end (a 16-byte group past
n_total, an element past the last comp_len / status / sidecar / dtinfo /
out_len) shows, which torch's rounded-up allocations hide.  Covers
fsehip_compress_blocks, fsehip_decompress_blocks (with and without the
sidecar), fsehip_build_sidecar, fsehip_build_dtables +
fsehip_decompress_blocks_dt, fsehip_decompress_streams, fsehip_generate and
fsehip_histogram_blocks, each also compared with the oracle (exact)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O

gpu = pytest.mark.gpu

GUARD_BYTES = 256
FILL = {"uint8": 0xA5, "int32": -99, "int64": -99}  # values no tested output can hold


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ---------------------------------------------------------------- the guard-band helper
def guarded(torch, n_elems, dtype, fill):
    """(whole, view): `view` is n_elems elements of `whole`, starts at a
    multiple of 256 bytes and has at least 256 bytes of `fill` on both sides
    (the view itself is filled too)."""
    item = torch.empty(0, dtype=dtype).element_size()
    pad = GUARD_BYTES // item
    body = (n_elems + pad - 1) // pad * pad
    whole = torch.full((pad + body + pad,), fill, dtype=dtype, device="cuda")
    assert whole.data_ptr() % GUARD_BYTES == 0
    view = whole[pad: pad + n_elems]
    assert view.numel() == n_elems and view.storage_offset() * item % GUARD_BYTES == 0
    return whole, view


def assert_guards(whole, view, fill, what=""):
    """Both bands of `whole` around `view` still hold `fill`."""
    lo, n = view.storage_offset(), view.numel()
    below, above = whole[:lo], whole[lo + n:]
    assert below.numel() * whole.element_size() >= GUARD_BYTES and above.numel() * whole.element_size() >= GUARD_BYTES
    assert bool((below == fill).all()), f"{what}: a store below the array"
    assert bool((above == fill).all()), f"{what}: a store past the array's last element"


def assert_all_written(view, fill, what=""):
    """An output the contract says is always written: no element still `fill`."""
    assert not bool((view == fill).any()), f"{what}: an element was never written"


def g8(torch, n):
    return guarded(torch, n, torch.uint8, FILL["uint8"])


def g32(torch, n):
    return guarded(torch, n, torch.int32, FILL["int32"])


def g64(torch, n):
    return guarded(torch, n, torch.int64, FILL["int64"])


def ptr(t):
    return C.c_void_p(t.data_ptr())


@gpu
def test_guard_helper_sees_a_stray_store(torch_cuda):
    """The helper itself: one element either side of a ragged view is caught,
    a store inside the view is not."""
    torch = torch_cuda
    for make, fill in ((g8, FILL["uint8"]), (g32, FILL["int32"]), (g64, FILL["int64"])):
        for n in (0, 1, 17, 4096):
            whole, view = make(torch, n)
            assert view.numel() == n and (n == 0 or view.data_ptr() % GUARD_BYTES == 0)
            view.fill_(1)
            assert_guards(whole, view, fill)
            lo = view.storage_offset()
            for stray in (lo - 1, lo + n):
                w2 = whole.clone()
                w2[stray] = 0
                with pytest.raises(AssertionError):
                    assert_guards(w2, w2[lo: lo + n], fill)
            if n:
                assert_all_written(view, fill)
                view[n - 1] = fill
                with pytest.raises(AssertionError):
                    assert_all_written(view, fill)


# ---------------------------------------------------------------- batched encode / decode at ragged ends
BLOCKS = [64, 1040, 65536]
FORMATS = [(2, 0), (2, 12), (2, 13), (1, 0)]  # (nstates, table_log): the <= 11, 12 and 13..15 kernel classes, 1-state
DATA = [(0, 0.155), (2, 0.0)]  # the bench's skewed generator; near-uniform (compressed ~ raw length)
CKPT = 64


def last_lengths(block):
    """Odd and even lengths, r % 16 on both sides of a 16-byte group, and the full block."""
    return [2, 15, 17, block - 15, block - 1, block]


def check_ragged_case(torch, block, r, fmt, data):
    """Three blocks, the last of r bytes: encode into guarded arrays, then
    decode through every route into a guarded `out` of exactly n_total bytes
    and a guarded status array."""
    from entropy_coders_amd import BlockCodec

    nstates, L = fmt
    kind, prob = data
    what = f"block {block} r {r} nstates {nstates} L {L} kind {kind}"
    sizes = [block, block, r]
    nb, n_total = 3, 2 * block + r
    blocks = [O.generate(kind, prob, 0x5EED0100 + block, b, s) for b, s in enumerate(sizes)]
    host = np.concatenate(blocks)
    # a case the oracle rejects fails here (an OracleError): none is skipped
    want = [O.compress2(s, L or None) if nstates == 2 else O.compress(s) for s in blocks]
    codec = BlockCodec(block_size=block, table_log=L, ckpt_interval=CKPT, nstates=nstates)
    assert codec.n_blocks(n_total) == nb
    src = torch.from_numpy(host).cuda()
    u8, i32, i64 = FILL["uint8"], FILL["int32"], FILL["int64"]

    # encode
    w_out, out = g8(torch, nb * codec.slot_bytes)
    w_len, comp_len = g32(torch, nb)
    w_bits, bits = g32(torch, nb)
    w_st, status = g32(torch, nb)
    w_side, side = g64(torch, nb * codec.side_per_block)
    cb = {"n_total": n_total, "out": out, "comp_len": comp_len, "payload_bits": bits, "sidecar": side,
          "status": status}
    codec.compress_into(src, cb)
    torch.cuda.synchronize()
    for w, v, f, name in ((w_out, out, u8, "slots"), (w_len, comp_len, i32, "comp_len"),
                          (w_bits, bits, i32, "payload_bits"), (w_st, status, i32, "status"),
                          (w_side, side, i64, "sidecar")):
        assert_guards(w, v, f, f"encode {name}, {what}")
    for v, name in ((comp_len, "comp_len"), (bits, "payload_bits"), (status, "status")):
        assert_all_written(v, i32, f"encode {name}, {what}")
    assert status.tolist() == [0] * nb, (what, status.tolist())
    for b in range(nb):
        assert codec.block_bytes(cb, b) == want[b][0], (what, b)
        assert int(bits[b]) == want[b][1], (what, b)

    # decode, every route
    def fresh():
        return g8(torch, n_total), g32(torch, nb)

    def verify(route, w_o, o, w_s, s):
        torch.cuda.synchronize()
        assert_guards(w_o, o, u8, f"{route} out, {what}")
        assert_guards(w_s, s, i32, f"{route} status, {what}")
        assert s.tolist() == [0] * nb, (route, what, s.tolist())
        assert torch.equal(o, src), (route, what)

    for use_sidecar in (True, False):
        (w_o, o), (w_s, s) = fresh()
        codec.decompress_into(cb, o, s, use_sidecar=use_sidecar)
        verify("sidecar" if use_sidecar else "sidecar-less", w_o, o, w_s, s)

    (w_o, o), (w_s, s) = fresh()
    w_so, side_out = g64(torch, nb * codec.side_per_block)
    p = codec.params()
    rc = codec.lib.fsehip_build_sidecar(C.byref(p), ptr(out), codec.slot_bytes, ptr(comp_len), ptr(o), n_total,
                                        ptr(side_out), ptr(s), codec._stream())
    assert rc == 0, (what, rc)
    verify("build_sidecar", w_o, o, w_s, s)
    assert_guards(w_so, side_out, i64, f"build_sidecar sidecar_out, {what}")

    per = int(codec.lib.fsehip_dtable_bytes(codec.max_table_log))
    w_dt, dt = g32(torch, nb * per // 4)
    w_info, info = g32(torch, nb)
    rc = codec.lib.fsehip_build_dtables(C.byref(p), ptr(out), codec.slot_bytes, ptr(comp_len), nb, ptr(dt), ptr(info),
                                        codec._stream())
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    assert_guards(w_dt, dt, i32, f"build_dtables tables, {what}")
    assert_guards(w_info, info, i32, f"build_dtables info, {what}")
    assert bool((info >= 0).all()), (what, info.tolist())
    (w_o, o), (w_s, s) = fresh()
    codec.decompress_dt_into(cb, {"dt": dt, "info": info}, o, s)
    verify("prebuilt tables", w_o, o, w_s, s)
    assert_guards(w_dt, dt, i32, f"decompress_blocks_dt tables, {what}")


@gpu
@pytest.mark.parametrize("data", DATA, ids=["skewed", "uniform"])
@pytest.mark.parametrize("fmt", FORMATS, ids=["2s-L0", "2s-L12", "2s-L13", "1s"])
@pytest.mark.parametrize("block", BLOCKS)
def test_ragged_ends(torch_cuda, block, fmt, data):
    for r in last_lengths(block):
        check_ragged_case(torch_cuda, block, r, fmt, data)


@gpu
def test_ragged_end_single_kernel_serial(torch_cuda):
    """The product's fallback when the deferred-symbol workspace cannot be
    had (the single-kernel serial decode, no sym_map_kernel), selected in a
    fresh child process on the diagnostics build as test_serial_deferred_symbols
    does: the same checks on one ragged case."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "entropy_coders_amd", "libfsehip_diag.so")):
        pytest.fail("libfsehip_diag.so missing: build it (make -C entropy_coders_amd diag / __graft_entry__.build())")
    env = dict(os.environ, FSEHIP_LIB="libfsehip_diag.so", FSEHIP_SERIAL_DEFER="0", PYTHONPATH=root)
    code = ("import torch, tests.test_gpu_guard_bands as t; import entropy_coders_amd._lib as L; "
            "assert L.LIB_PATH.endswith('libfsehip_diag.so'); "
            "t.check_ragged_case(torch, 1040, 17, (2, 0), (0, 0.155)); print('child-ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child-ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---------------------------------------------------------------- fsehip_decompress_streams
STREAM_LENGTHS = [3, 4, 5, 7, 15, 16, 17, 31, 33, 48, 63, 64, 65, 100, 143, 144, 145, 177, 199, 200,
                  4093, 4096, 4099, 4112, 4113, 4200]


@pytest.fixture(scope="module")
def crate_streams():
    """Oracle streams of STREAM_LENGTHS raw bytes in both formats (7 symbols
    for the short ones, the bench's skewed generator from 64 bytes on)."""
    rng = np.random.default_rng(0x57E4)
    alpha = np.array([3, 9, 27, 81, 128, 200, 255], dtype=np.uint8)
    raws = []
    for i, n in enumerate(STREAM_LENGTHS):
        raw = O.generate(0, 0.155, 0x5EED0200, i, n) if n >= 64 and i % 2 else alpha[rng.integers(0, 7, n)]
        raw[:2] = [3, 9]  # two symbols at least: the crate encodes it, and its decoder terminates
        raws.append(raw)
    return raws, {2: [O.compress2(r)[0] for r in raws], 1: [O.compress(r)[0] for r in raws]}


@gpu
@pytest.mark.parametrize("max_table_log", [11, 12])  # deferred symbols + sym_map_kernel; the serial kernel alone
@pytest.mark.parametrize("stride", [64, 144, 4112])
@pytest.mark.parametrize("nstates", [2, 1])
def test_decompress_streams_guarded(torch_cuda, crate_streams, nstates, stride, max_table_log):
    torch = torch_cuda
    from entropy_coders_amd import load
    from entropy_coders_amd._lib import STATUS

    raws, comp = crate_streams
    streams = comp[nstates]
    n = len(streams)
    ref = O.decompress2 if nstates == 2 else O.decompress
    want = []
    for x in streams:
        try:
            want.append(ref(x, stride))
        except O.OracleError as e:
            want.append(e.code)
    fits = [not isinstance(w, str) for w in want]
    assert any(fits) and "DST_TOO_SMALL" in want
    assert any(f and len(w) == stride for f, w in zip(fits, want))  # some end exactly at the stride
    in_stride = (max(len(x) for x in streams) + 255) // 256 * 256
    host = np.zeros(n * in_stride, dtype=np.uint8)
    for i, x in enumerate(streams):
        host[i * in_stride: i * in_stride + len(x)] = np.frombuffer(x, dtype=np.uint8)
    d_in = torch.from_numpy(host).cuda()
    lens = torch.tensor([len(x) for x in streams], dtype=torch.int32, device="cuda")
    w_out, out = g8(torch, n * stride)
    w_len, out_len = g32(torch, n)
    w_st, status = g32(torch, n)
    rc = load().fsehip_decompress_streams(nstates, max_table_log, ptr(d_in), in_stride, ptr(lens), n, ptr(out), stride,
                                          ptr(out_len), ptr(status),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert_guards(w_out, out, FILL["uint8"], "out")
    assert_guards(w_len, out_len, FILL["int32"], "out_len")
    assert_guards(w_st, status, FILL["int32"], "status")
    assert_all_written(out_len, FILL["int32"], "out_len")
    assert_all_written(status, FILL["int32"], "status")
    ho, ol, st = out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
    for i, w in enumerate(want):
        assert 0 <= ol[i] <= stride, (i, ol[i])
        if isinstance(w, str):
            assert STATUS[int(st[i])] == w, (i, w, st[i])
        else:
            assert st[i] == 0 and ol[i] == len(w), (i, st[i], ol[i], len(w))
            assert ho[i * stride: i * stride + len(w)].tobytes() == w, i


# ---------------------------------------------------------------- fsehip_generate
@gpu
@pytest.mark.parametrize("kind,prob", [(0, 0.155), (1, 0.0), (2, 0.0)])
@pytest.mark.parametrize("block,n_total", [(65536, 1), (65536, 15), (65536, 16), (65536, 17), (65536, 65536 + 9),
                                           (48, 100)])
def test_generate_guarded(torch_cuda, block, n_total, kind, prob):
    torch = torch_cuda
    from entropy_coders_amd import load

    seed = 0x5EED0300 + n_total
    w_out, out = g8(torch, n_total)
    rc = load().fsehip_generate(kind, prob, seed, block, ptr(out), n_total,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert_guards(w_out, out, FILL["uint8"], "generate")
    got = out.cpu().numpy()
    for b in range((n_total + block - 1) // block):
        n = min(block, n_total - b * block)
        assert np.array_equal(got[b * block: b * block + n], O.generate(kind, prob, seed, b, n)), b


# ---------------------------------------------------------------- fsehip_histogram_blocks
HIST_SHAPES = [(16, 16 * 5 + 1), (48, 48 * 3 + 47), (4096, 4096 * 4 + 15), (65536, 65536 * 2 + 1), (65536, 0),
               (65536, 7)]


@gpu
@pytest.mark.parametrize("block,n_total", HIST_SHAPES)
def test_histogram_blocks(torch_cuda, block, n_total):
    """histogram::count per block against np.bincount and 1 + the largest
    symbol (1 for an empty input), multi-block with a ragged last block."""
    torch = torch_cuda
    from test_gpu_fuzz import _block  # seeded random distributions

    from entropy_coders_amd import load

    lib = load()
    rng = np.random.default_rng(0x4157 + block + n_total)
    nb = max(1, (n_total + block - 1) // block)
    sizes = [min(block, n_total - b * block) for b in range(nb)]
    blocks = [_block(rng, s) if s else np.zeros(0, np.uint8) for s in sizes]
    if (block, n_total) == HIST_SHAPES[1]:
        blocks[1] = np.zeros(block, np.uint8)  # all zeros: table_len 1
    if (block, n_total) == HIST_SHAPES[2]:
        blocks[2] = blocks[2].copy()
        blocks[2][-1] = 255  # the largest symbol: table_len 256
        assert blocks[2].max() == 255
    host = np.concatenate(blocks + [np.zeros(16, np.uint8)])  # (never empty: the call takes no null pointer)
    src = torch.from_numpy(host).cuda()
    want_counts = np.concatenate([np.bincount(s, minlength=256) for s in blocks]).astype(np.int64)
    want_tl = [int(s.max()) + 1 if len(s) else 1 for s in blocks]
    hs = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_tl in (True, False):
        w_c, counts = g32(torch, nb * 256)
        w_t, tl = g32(torch, nb)
        rc = lib.fsehip_histogram_blocks(ptr(src), n_total, block, ptr(counts), ptr(tl) if with_tl else None, hs)
        assert rc == 0
        torch.cuda.synchronize()
        assert_guards(w_c, counts, FILL["int32"], "counts")
        assert_guards(w_t, tl, FILL["int32"], "table_len")
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), want_counts), with_tl
        if with_tl:
            assert tl.tolist() == want_tl
        else:  # a null d_table_len: nothing of that array is touched
            assert tl.tolist() == [FILL["int32"]] * nb


def test_histogram_blocks_bad_args():
    """Call-level checks that return before any device use (no GPU needed):
    several blocks of a size that is no multiple of 16, and null pointers."""
    from entropy_coders_amd import load
    from entropy_coders_amd._lib import STATUS

    lib = load()
    a, b, c = (C.c_void_p(x) for x in (0x1000, 0x2000, 0x3000))  # never dereferenced
    assert STATUS[lib.fsehip_histogram_blocks(a, 100, 49, b, c, None)] == "BAD_ARG"
    assert STATUS[lib.fsehip_histogram_blocks(a, 8 * 65536, 65536 + 8, b, c, None)] == "BAD_ARG"
    assert STATUS[lib.fsehip_histogram_blocks(None, 100, 16, b, c, None)] == "BAD_ARG"
    assert STATUS[lib.fsehip_histogram_blocks(a, 100, 16, None, c, None)] == "BAD_ARG"
