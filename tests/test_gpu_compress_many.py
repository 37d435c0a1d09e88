"""Batched compression of many variable-length buffers in one call:
fse_compress2_many / fse_compress_many (host buffers) and
fsehip_compress_streams (device buffers, a descriptor per stream), each
stream checked against the oracle's fse_compress2 / fse_compress /
fse_compress2_log (lib.rs:146-183, 112-143): exact bytes, payload bits and
statuses, and no store outside a stream's own output window."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

LENGTHS = [2, 3, 4, 5, 15, 16, 17, 31, 33, 255, 4096, 8193, 65535, 65536, 65537, 100001]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module", autouse=True)
def rank_fallbacks_stay_zero(torch_cuda):
    """No table of this file's calls fell back to the peer-mask ranks."""
    from entropy_coders_amd import load

    lib = load()
    c = (C.c_uint32 * 3)()
    assert lib.fsehip_rank_fallbacks(0, C.byref(c), 1) == 0  # read and reset
    yield
    assert lib.fsehip_rank_fallbacks(0, C.byref(c), 0) == 0
    assert list(c) == [0, 0, 0]


def _data(rng, n, kind):
    """Three alphabets: skewed (the bench's C2 generator), 7 symbols, near-uniform."""
    if kind == 0:
        return O.generate(0, 0.155, 0x5EED0002, int(rng.integers(1 << 20)), n)
    if kind == 1:
        return np.array([3, 9, 27, 81, 128, 200, 255], dtype=np.uint8)[rng.integers(0, 7, n)]
    return rng.integers(0, 250, n).astype(np.uint8)


def _ref(src, nstates=2, log2=None):
    """The oracle's (bytes, payload bits), or the name of its status."""
    try:
        return O.compress2(src, log2) if nstates == 2 else O.compress(src)
    except O.OracleError as e:
        return e.code


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(0xC0DE)
    # (a few skewed bytes are all zeros, which the crate refuses: the short ones take the other alphabets)
    bufs = [_data(rng, n, i % 3 if n >= 255 else 1 + i % 2) for i, n in enumerate(LENGTHS)]
    return bufs, {ns: [_ref(b, ns) for b in bufs] for ns in (1, 2)}


@pytest.fixture(scope="module")
def c2_streams():
    """1,000 64 KiB C2 streams and their oracle outputs, computed once."""
    bufs = [O.generate(0, 0.155, 0x5EED0002, i, 65536) for i in range(1000)]
    return bufs, [O.compress2(b) for b in bufs]


# 1 ---------------------------------------------------------------- exact bytes
@pytest.mark.parametrize("route", ["many", "streams"])
@pytest.mark.parametrize("nstates", [2, 1])
def test_mixed_lengths_exact(torch_cuda, mixed, nstates, route):
    from entropy_coders_amd import compress2_many, compress_streams, decompress2_many

    bufs, want = mixed
    got = compress2_many(bufs, nstates=nstates) if route == "many" else compress_streams(bufs, nstates=nstates)
    assert len(got) == len(bufs)
    for n, g, w in zip(LENGTHS, got, want[nstates]):
        assert not isinstance(w, str), (n, w)  # every length from 2 up is a valid stream
        assert g == w, (n, nstates, route)
    back = decompress2_many([g[0] for g in got], 100016, nstates=nstates)
    for b, r in zip(bufs, back):
        assert r == b.tobytes()


# 2 ---------------------------------------------------------------- statuses isolate
@pytest.mark.parametrize("nstates", [2, 1])
def test_statuses_isolate(torch_cuda, nstates):
    from entropy_coders_amd import STATUS, compress2_many, compress_streams

    rng = np.random.default_rng(0x57A7)
    good = [_data(rng, n, k) for n, k in ((777, 0), (4096, 1), (65536, 2), (12345, 0), (100, 1), (65536, 0))]
    one = np.array([7], dtype=np.uint8)
    bufs = [good[0], b"", good[1], one, good[2], np.zeros(64, np.uint8), good[3], np.zeros(65536, np.uint8),
            good[4], (None, 100), good[5]]
    want = [_ref(b, nstates) if not isinstance(b, tuple) else "BAD_ARG" for b in bufs]
    assert [w for w in want if isinstance(w, str)] == ["EMPTY", "TOO_SHORT", "ALL_ZERO_SYMBOL0", "ALL_ZERO_SYMBOL0",
                                                       "BAD_ARG"]
    dst, lens, bits, st = compress2_many(bufs, nstates=nstates, raw=True)
    stride = len(dst) // len(bufs)
    for i, w in enumerate(want):
        if isinstance(w, str):
            assert STATUS[int(st[i])] == w and lens[i] == 0 and bits[i] == 0, (i, w)
        else:
            assert st[i] == 0 and dst[i * stride: i * stride + int(lens[i])].tobytes() == w[0] and bits[i] == w[1], i
    # the device call: the same batch without the null pointer
    dbufs = [b for b in bufs if not isinstance(b, tuple)]
    dgot = compress_streams(dbufs, nstates=nstates)
    assert dgot == [_ref(b, nstates) for b in dbufs]
    st, cl, _, _, _ = compress_streams(dbufs, nstates=nstates, raw=True)
    assert all(cl[i] == 0 for i in range(len(dbufs)) if st[i] != 0)


# 3 ---------------------------------------------------------------- exact DST_TOO_SMALL
def test_dst_too_small_is_exact(torch_cuda):
    from entropy_coders_amd import STATUS, compress2_many

    rng = np.random.default_rng(0xD57)
    bufs = [_data(rng, n, k) for n, k in ((100, 0), (65536, 2), (4096, 1), (65536, 2), (30000, 0), (65536, 0))]
    bufs.append(np.array([0, 9], dtype=np.uint8))  # 2 bytes in, 9 bytes out
    want = [O.compress2(b) for b in bufs]
    stride = max(len(w[0]) for w in want) - 1
    n_fail = sum(len(w[0]) > stride for w in want)
    assert 1 <= n_fail < len(bufs)
    dst = np.full(len(bufs) * stride + 4096, 0xEE, dtype=np.uint8)
    _, lens, bits, st = compress2_many(bufs, dst_stride=stride, raw=True, dst=dst)
    for i, w in enumerate(want):
        win = dst[i * stride: (i + 1) * stride]
        if len(w[0]) > stride:
            assert STATUS[int(st[i])] == "DST_TOO_SMALL" and lens[i] == 0, i
            assert (win == 0xEE).all(), i
        else:
            assert st[i] == 0 and win[: int(lens[i])].tobytes() == w[0] and bits[i] == w[1], i
            assert (win[int(lens[i]):] == 0xEE).all(), i
    assert (dst[len(bufs) * stride:] == 0xEE).all()
    # the 2-byte input is 9 bytes: 8 do not hold it, 9 do
    two = [bufs[-1], bufs[-1], bufs[0]]
    assert len(want[-1][0]) == 9
    for stride, code in ((8, "DST_TOO_SMALL"), (9, "OK")):
        dst = np.full(3 * stride + 64, 0xEE, dtype=np.uint8)
        _, lens, _, st = compress2_many(two, dst_stride=stride, raw=True, dst=dst)
        assert [STATUS[int(x)] for x in st] == [code, code, "DST_TOO_SMALL"]
        if code == "OK":
            assert dst[:9].tobytes() == want[-1][0] and dst[9:18].tobytes() == want[-1][0] and list(lens) == [9, 9, 0]
            assert (dst[18:] == 0xEE).all()
        else:
            assert (dst == 0xEE).all() and list(lens) == [0, 0, 0]


# 4 ---------------------------------------------------------------- device bounds
def _check_bounds(bufs, want, caps, nstates, table_log, untouched=False):
    from entropy_coders_amd import STATUS, compress_streams

    st, cl, pb, out, desc = compress_streams(bufs, nstates=nstates, table_log=table_log, out_caps=caps, raw=True)
    canary = np.ones(len(out), dtype=bool)
    for (_, oo, _, cap) in desc:
        canary[oo: oo + cap] = False
    assert canary.sum() >= 64 * len(bufs)
    assert (out[canary] == 0xA5).all(), "a store left its stream's output region"
    codes = []
    for i, (w, cap) in enumerate(zip(want, caps)):
        oo = desc[i][1]
        codes.append(STATUS[int(st[i])])
        if len(w[0]) <= cap:
            assert st[i] == 0 and out[oo: oo + int(cl[i])].tobytes() == w[0] and int(pb[i]) == w[1], (i, cap)
        else:
            assert codes[-1] == "DST_TOO_SMALL" and cl[i] == 0, (i, cap)
            if untouched:  # the header alone does not fit: nothing is written
                assert (out[oo: oo + cap] == 0xA5).all()
    return codes


@pytest.mark.parametrize("nstates", [2, 1])
def test_device_bounds(torch_cuda, nstates):
    rng = np.random.default_rng(0xB0B + nstates)
    src = [_data(rng, n, i % 3) for i, n in enumerate([2, 33, 255, 1000, 4096, 4097, 5000, 65536, 65537])]
    ref = [_ref(b, nstates) for b in src]
    bufs, want, caps = [], [], []
    for b, w in zip(src, ref):
        for cap in (len(w[0]), len(w[0]) - 1, 16):
            bufs.append(b)
            want.append(w)
            caps.append(cap)
    assert {c % 4 for c in caps} == {0, 1, 2, 3}  # the region's last partial word, every width
    codes = _check_bounds(bufs, want, caps, nstates, 0)
    k = 3 * 4  # the 4096-byte stream: exact, one short, 16
    assert codes[k: k + 3] == ["OK", "DST_TOO_SMALL", "DST_TOO_SMALL"]
    # a capacity below the header's length: nothing is written at all
    tiny = _check_bounds([src[8]] * 3, [ref[8]] * 3, [0, 3, 15], nstates, 0, untouched=True)  # ~250 symbols: a long header
    assert tiny == ["DST_TOO_SMALL"] * 3


def test_device_bounds_table_log_13(torch_cuda):
    """At table log 13 the spread's 8 KiB symbol array must not live in a
    region of ~1 KiB: in-slot scratch would overrun it."""
    rng = np.random.default_rng(0x13)
    src = [_data(rng, 1024, i % 3) for i in range(6)]
    ref = [O.compress2(b, 13) for b in src]
    bufs, want, caps = [], [], []
    for b, w in zip(src, ref):
        for cap in (len(w[0]), len(w[0]) - 1, 16):
            bufs.append(b)
            want.append(w)
            caps.append(cap)
    codes = _check_bounds(bufs, want, caps, 2, 13)
    assert codes == ["OK", "DST_TOO_SMALL", "DST_TOO_SMALL"] * 6


# 5 ---------------------------------------------------------------- table-log classes
@pytest.mark.parametrize("L", [9, 12, 13, 15])
def test_table_log_classes(torch_cuda, L):
    from entropy_coders_amd import compress_streams

    rng = np.random.default_rng(0x7AB + L)
    bufs = [_data(rng, n, k) for n in (4096, 65536) for k in (0, 1, 2)]
    bufs += [O.generate(0, 0.5, 99, 0, 65536), O.generate(0, 0.02, 7, 0, 4096)]
    # two streams that end in two rare symbols: their seeds pass new_first_symbol at table log 15 too
    for b in (bufs[0], bufs[4]):
        b = b.copy()
        b[-2:] = [251, 252]
        bufs.append(b)
    want = [_ref(b, 2, L) for b in bufs]
    got = compress_streams(bufs, table_log=L)
    assert got == want, [(g if isinstance(g, str) else len(g[0]), w if isinstance(w, str) else len(w[0]))
                         for g, w in zip(got, want)]
    if L == 15:
        assert "ENCODER_INIT" in want  # the tableLog-15 panic of new_first_symbol
    assert sum(not isinstance(w, str) for w in want) >= 2
    # a table log above the kernel bound asked for: UNSUPPORTED per stream
    if L >= 12:
        assert compress_streams(bufs[:2], table_log=L, max_table_log=11) == ["UNSUPPORTED"] * 2


# 6 ---------------------------------------------------------------- misaligned offsets
def test_misaligned_offsets_are_that_streams_bad_arg(torch_cuda):
    torch = torch_cuda
    from entropy_coders_amd import STATUS, load
    from entropy_coders_amd._lib import StreamDesc

    rng = np.random.default_rng(0xA11)
    bufs = [_data(rng, 3000, i % 3) for i in range(5)]
    want = [O.compress2(b) for b in bufs]
    host = np.zeros(5 * 3008 + 64, dtype=np.uint8)
    desc = (StreamDesc * 5)()
    skew_src, skew_out = {1: 8}, {3: 4}  # stream 1: src_off % 16 = 8; stream 3: out_off % 16 = 4
    for i, b in enumerate(bufs):
        so = i * 3008 + skew_src.get(i, 0)
        host[so: so + 3000] = b
        desc[i] = StreamDesc(so, i * 4096 + skew_out.get(i, 0), 3000, 4000)
    dev = torch.device("cuda")
    d_src = torch.from_numpy(host).to(dev)
    d_desc = torch.from_numpy(np.frombuffer(bytes(desc), dtype=np.uint8).copy()).to(dev)
    out = torch.full((5 * 4096,), 0xA5, dtype=torch.uint8, device=dev)
    cl = torch.full((5,), 7, dtype=torch.int32, device=dev)
    pb = torch.zeros(5, dtype=torch.int32, device=dev)
    st = torch.zeros(5, dtype=torch.int32, device=dev)
    rc = load().fsehip_compress_streams(2, 0, 0, C.c_void_p(d_src.data_ptr()), C.c_void_p(d_desc.data_ptr()), 5,
                                        C.c_void_p(out.data_ptr()), C.c_void_p(cl.data_ptr()),
                                        C.c_void_p(pb.data_ptr()), C.c_void_p(st.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    ho, cl, st = out.cpu().numpy(), cl.cpu().numpy(), st.cpu().numpy()
    assert [STATUS[int(x)] for x in st] == ["OK", "BAD_ARG", "OK", "BAD_ARG", "OK"]
    for i in (0, 2, 4):
        assert ho[i * 4096: i * 4096 + int(cl[i])].tobytes() == want[i][0]
    for i in (1, 3):
        assert cl[i] == 0 and (ho[i * 4096: (i + 1) * 4096] == 0xA5).all()


# 7 ---------------------------------------------------------------- the batch split does not show
def test_batch_split_does_not_show(torch_cuda):
    from entropy_coders_amd import compress2_many, load

    rng = np.random.default_rng(0x5917)
    sizes = rng.integers(1 << 20, 3 << 20, 40)
    bufs = [rng.integers(0, 12 + 6 * (i % 5), int(n), dtype=np.uint8) for i, n in enumerate(sizes)]
    lib = load()
    lib.fsehipx_compress_many_stage.restype = C.c_uint64
    lib.fsehipx_compress_many_stage.argtypes = [C.c_uint64]
    stride = int(lib.fsehip_stream_out_bytes(3 << 20, 11))
    prev = lib.fsehipx_compress_many_stage(16 << 20)  # the product's cap is 512 MiB: ~8 batches instead of 1
    try:
        d1, l1, b1, s1 = compress2_many(bufs, dst_stride=stride, raw=True)
        halves = [compress2_many(h, dst_stride=stride, raw=True) for h in (bufs[:20], bufs[20:])]
    finally:
        lib.fsehipx_compress_many_stage(prev)
    d0, l0, b0, s0 = compress2_many(bufs, dst_stride=stride, raw=True)  # one batch
    l2 = np.concatenate([h[1] for h in halves])
    b2 = np.concatenate([h[2] for h in halves])
    s2 = np.concatenate([h[3] for h in halves])
    d2 = np.concatenate([h[0] for h in halves])
    assert (s1 == 0).all() and (s2 == 0).all() and (s0 == 0).all()
    assert (l1 == l2).all() and (b1 == b2).all() and (l1 == l0).all() and (b1 == b0).all()
    for i in range(40):
        a = d1[i * stride: i * stride + int(l1[i])]
        assert (a == d2[i * stride: i * stride + int(l1[i])]).all(), i
        assert (a == d0[i * stride: i * stride + int(l1[i])]).all(), i
    for i in (0, 19, 20, 39):
        w = O.compress2(bufs[i])
        assert d1[i * stride: i * stride + int(l1[i])].tobytes() == w[0] and b1[i] == w[1]


# 8 ---------------------------------------------------------------- counts
@pytest.mark.parametrize("count", [1, 2, 3, 33, 1000])
def test_counts(torch_cuda, c2_streams, count):
    from entropy_coders_amd import compress2_many

    bufs, want = c2_streams
    got = compress2_many(bufs[:count])
    assert len(got) == count
    for i in range(count):
        assert got[i] == want[i], i
