"""Caller-built histograms and tables through the building blocks of
include/fsehip.h section 1b, and histogram_new beyond one counting segment.

Every other GPU test of normalisation, the NCount header and the table
builds starts from the bytes of a sampled block.  Here the structs are the
caller's (tests/caller_cases.py): sizes up to 2^32 - 1 whose u32 products
wrap, every exit of normalize / normalize_slow a consistent histogram
reaches (FSE_ERR_CURSED among them), ties, the rounding table's edges, and
normalised tables that TryFrom accepts but normalisation never produces,
through norm_histogram_write / read (every truncation), encode_table_new /
decode_table_new and the stream decoders.  Expected values are exact and come
from the C oracle and the Python spec, never from the library;
tests/test_caller_cases.py holds the two to each other on the same cases."""
import ctypes as C
import functools

import numpy as np
import pytest

import caller_cases as CC
import shared_ref as R
from oracle import oracle as O
from oracle import spec
from test_gpu_guard_bands import FILL, assert_all_written, assert_guards, g8, g32, g64, ptr

pytestmark = pytest.mark.gpu


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


def status_name(rc):
    from entropy_coders_amd._lib import STATUS

    return STATUS.get(int(rc), str(int(rc)))


def o_hist(counts, size, table_len):
    h = O.Hist()
    for i, c in enumerate(counts):
        h.counts[i] = c
    h.size, h.table_len = size, table_len
    return h


def o_norm(table, L, table_len):
    nh = O.Norm()
    for i, v in enumerate(table):
        nh.norm[i] = v
    nh.log2, nh.table_len = L, table_len
    return nh


def dev_hist(counts, size, table_len):
    from entropy_coders_amd._lib import Histogram

    h = Histogram()
    for i, c in enumerate(counts):
        h.counts[i] = c
    h.size, h.table_len = size, table_len
    return h


def dev_norm(table, L, table_len):
    from entropy_coders_amd._lib import NormHistogram

    nh = NormHistogram()
    for i, v in enumerate(table):
        nh.norm[i] = v
    nh.log2, nh.table_len = L, table_len
    return nh


def outcome(fn, err):
    """fn()'s value, or the status name of the error it raises."""
    try:
        return fn()
    except err as e:
        return e.code


# ---------------------------------------------------------------- 1. normalise a caller's struct
def expected_norm(counts, size, tl, log2):
    def run():
        nh, _ = O.normalize(o_hist(counts, size, tl), log2)
        return list(nh.norm), nh.log2, nh.table_len

    return outcome(run, O.OracleError)


@pytest.mark.parametrize("case", CC.HIST_CASES, ids=[c[0] for c in CC.HIST_CASES])
def test_normalize_callers_struct(torch_cuda, case):
    from entropy_coders_amd import FseError, normalize

    name, counts, size, tl, log2, label = case
    want = expected_norm(counts, size, tl, log2)
    assert (want == "CURSED") == label.endswith("cursed")

    def run():
        nh = normalize(dev_hist(counts, size, tl), log2)
        return list(nh.norm), nh.log2, nh.table_len

    got = outcome(run, FseError)
    print(name, label, want if isinstance(want, str) else (want[1], want[2]))
    assert got == want, (name, label)


@pytest.mark.parametrize("case", CC.OPTIMAL_CASES, ids=[c[0] for c in CC.OPTIMAL_CASES])
def test_normalize_optimal_callers_struct(torch_cuda, case):
    from entropy_coders_amd import FseError, normalize_optimal

    name, counts, size, tl = case
    want = expected_norm(counts, size, tl, O.optimal_log2(o_hist(counts, size, tl)))

    def run():
        nh = normalize_optimal(dev_hist(counts, size, tl))
        return list(nh.norm), nh.log2, nh.table_len

    assert outcome(run, FseError) == want, name


# ---------------------------------------------------------------- 2. the same branches inside the encoder
ENC_CASES = [c for c in CC.HIST_CASES if CC.consistent(c) and c[2] <= 65536]


@functools.lru_cache(maxsize=None)
def block_of(name):
    """A block with exactly the case's byte counts, shuffled with a fixed seed."""
    case = next(c for c in ENC_CASES if c[0] == name)
    raw = np.repeat(np.arange(256, dtype=np.uint8), np.asarray(case[1], dtype=np.int64))
    np.random.default_rng(0xB10C5).shuffle(raw)
    assert np.array_equal(np.bincount(raw, minlength=256), case[1])
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def neighbours(block):
    """Two full blocks of other shapes (256 symbols; 7 symbols) for the batch."""
    a = O.generate(2, 0.0, 0x5EEDCA11, 0, block) + np.uint8(8)
    b = O.generate(0, 0.77, 0x5EEDCA11, 1, block)
    return a, b


def oracle_comp(raw, nstates, log2):
    fn = O.compress2 if nstates == 2 else O.compress
    return outcome(lambda: fn(raw, log2), O.OracleError)


@pytest.mark.parametrize("case", ENC_CASES, ids=[c[0] for c in ENC_CASES])
def test_encoder_takes_the_same_branch(torch_cuda, case):
    torch = torch_cuda
    from entropy_coders_amd import BlockCodec, FseError, compress2_log, compress_streams

    name, counts, size, tl, log2, label = case
    raw = block_of(name)
    forced = min(max(log2, 5), 15)  # the crate's clamp; 0 in the batched parameters would ask for optimal_log2
    want = {ns: oracle_comp(raw, ns, log2) for ns in (2, 1)}
    assert want == {ns: oracle_comp(raw, ns, forced) for ns in (2, 1)}
    print(name, label, {ns: w if isinstance(w, str) else len(w[0]) for ns, w in want.items()})

    # fse_compress2 on the host, at the requested log as given
    assert outcome(lambda: compress2_log(raw, log2), FseError) == want[2], name

    block = (size + 15) // 16 * 16
    n1, n2 = neighbours(block)
    for ns in (2, 1):
        nwant = [oracle_comp(x, ns, forced) for x in (n1, n2)]
        # fsehip_compress_blocks: alone, then third in a batch of three, outputs between guard bands
        for batch in ([raw], [n1, n2, raw]):
            nb = len(batch)
            expect = ([] if nb == 1 else nwant) + [want[ns]]
            codec = BlockCodec(block_size=block, table_log=forced, ckpt_interval=64, nstates=ns)
            host = np.concatenate(batch)
            src = torch.from_numpy(host).cuda()
            w_out, out = g8(torch, nb * codec.slot_bytes)
            w_len, comp_len = g32(torch, nb)
            w_bits, bits = g32(torch, nb)
            w_st, status = g32(torch, nb)
            w_side, side = g64(torch, nb * codec.side_per_block)
            cb = {"n_total": len(host), "out": out, "comp_len": comp_len, "payload_bits": bits, "sidecar": side,
                  "status": status}
            codec.compress_into(src, cb)
            torch.cuda.synchronize()
            for w, v, f, what in ((w_out, out, "uint8", "slots"), (w_len, comp_len, "int32", "comp_len"),
                                  (w_bits, bits, "int32", "payload_bits"), (w_st, status, "int32", "status"),
                                  (w_side, side, "int64", "sidecar")):
                assert_guards(w, v, FILL[f], f"{name} ns {ns} nb {nb} {what}")
            assert_all_written(status, FILL["int32"], "status")
            st = status.tolist()
            for b, e in enumerate(expect):
                if isinstance(e, str):
                    assert status_name(st[b]) == e, (name, ns, nb, b)
                else:
                    assert st[b] == 0, (name, ns, nb, b, status_name(st[b]))
                    assert codec.block_bytes(cb, b) == e[0], (name, ns, nb, b)
                    assert int(bits[b]) == e[1], (name, ns, nb, b)
        # fsehip_compress_streams: the block third among three streams
        got = compress_streams([n1, n2, raw], nstates=ns, table_log=forced)
        assert got == nwant + [want[ns]], (name, ns)


# ---------------------------------------------------------------- 3. header bytes, truncation, tables
ALL_TABLES = [(n, t, R.try_from(t)[2]) for n, t in CC.TABLE_CASES] + CC.STRUCT_CASES
TABLE_IDS = [c[0] for c in ALL_TABLES]


@pytest.mark.parametrize("case", ALL_TABLES, ids=TABLE_IDS)
def test_header_bytes(torch_cuda, case):
    from entropy_coders_amd import norm_histogram_read, norm_histogram_write

    name, table, tl = case
    norm, L, _ = R.try_from(table)
    want = O.header_write(o_norm(table, L, tl))
    got, bits = norm_histogram_write(dev_norm(table, L, tl))
    assert got == want, name
    assert bits == spec.header_bits(norm, L, tl) and (bits + 7) // 8 == len(want), name
    data = want + bytes(range(7))
    back, used = norm_histogram_read(data)
    ref, rused = O.header_read(data)
    assert used == rused == len(want)
    assert (list(back.norm), back.log2, back.table_len) == (list(ref.norm), ref.log2, ref.table_len), name
    assert list(back.norm) == norm and back.log2 == L


def read_outcome_oracle(data):
    def run():
        nh, used = O.header_read(data)
        return list(nh.norm), nh.log2, nh.table_len, used

    return outcome(run, O.OracleError)


@pytest.mark.parametrize("case", CC.TABLE_CASES, ids=[c[0] for c in CC.TABLE_CASES])
def test_header_truncation(torch_cuda, case):
    """norm_histogram_read on every prefix of a header up to 64 bytes (the
    last 16 prefix lengths of a longer one), the header itself with no byte
    behind it included: status, consumed and the table are the oracle's."""
    from entropy_coders_amd import FseError, norm_histogram_read

    name, table = case
    norm, L, tl = R.try_from(table)
    head = O.header_write(o_norm(table, L, tl))
    seen = set()
    for k in CC.prefix_lengths(len(head)):
        want = read_outcome_oracle(head[:k])

        def run():
            nh, used = norm_histogram_read(head[:k])
            return list(nh.norm), nh.log2, nh.table_len, used

        got = outcome(run, FseError)
        assert got == want, (name, k, len(head))
        seen.add(want if isinstance(want, str) else "OK")
    print(name, len(head), sorted(seen))
    assert "OK" in seen


@pytest.mark.parametrize("case", ALL_TABLES, ids=TABLE_IDS)
def test_tables_from_callers_struct(torch_cuda, case):
    """encode_table_new / decode_table_new, compared as
    test_gpu_blocks.test_encode_decode_tables compares them."""
    from entropy_coders_amd import decode_table_new, encode_table_new

    name, table, tl = case
    L = R.try_from(table)[1]
    nh_o, nh = o_norm(table, L, tl), dev_norm(table, L, tl)
    log2, st, dnb, dfs, spread = O.ctable(nh_o)
    et = encode_table_new(nh)
    size = 1 << log2
    assert et.table_log == log2 == L
    assert np.array_equal(np.ctypeslib.as_array(et.table)[:size], st), name
    assert np.array_equal(np.ctypeslib.as_array(et.symbols)[:size], spread), name
    tt = np.ctypeslib.as_array(et.symbol_tt)
    assert [t[0] for t in tt] == list(dnb) and [t[1] for t in tt] == list(dfs), name
    log2, ns, sym, nb = O.dtable_nh(nh_o)
    dt = decode_table_new(nh)
    e = np.ctypeslib.as_array(dt.table)[:size]
    assert dt.table_log == log2
    assert np.array_equal(e["new_state"], ns) and np.array_equal(e["symbol"], sym), name
    assert np.array_equal(e["num_bits"], nb), name
    big = any(v >= 1 << (log2 - 1) for v in table[:tl])
    assert dt.fast_mode == (0 if big else 1), name


def test_fast_mode_boundary_is_covered():
    modes = {n: max(t) >= 1 << (R.try_from(t)[1] - 1) for n, t in CC.TABLE_CASES}
    assert modes["half_L6"] and modes["half_L12"] and not modes["half_minus_one_L6"] and not modes["half_minus_one_L12"]


# ---------------------------------------------------------------- streams of the crate's Encoder against such tables
def kernel_class(L):
    return 11 if L <= 11 else L


def stream_groups():
    """The written streams by (nstates, kernel class)."""
    groups = {}
    for r in CC.table_streams():
        if r["stream"] is not None:
            groups.setdefault((r["nstates"], kernel_class(r["log"])), []).append(r)
    return groups


GROUPS = sorted({(ns, kernel_class(R.try_from(t)[1])) for _, t in CC.TABLE_CASES for ns in (2, 1)})


def test_streams_exist_for_every_group():
    groups = stream_groups()
    assert set(groups) == set(GROUPS)
    assert {r["n"] for g in groups.values() for r in g} == set(CC.STREAM_LENGTHS)
    for r in CC.table_streams():  # what the crate's Encoder cannot write is its own panic, nothing else
        assert r["stream"] is not None or r["status"] == "ENCODER_INIT", (r["name"], r["status"])


@pytest.mark.parametrize("group", GROUPS, ids=[f"{ns}s-L{c}" for ns, c in GROUPS])
def test_streams_host_many(torch_cuda, group):
    """fse_decompress2_many / fse_decompress_many."""
    from entropy_coders_amd import decompress2_many

    recs = stream_groups()[group]
    got = decompress2_many([r["stream"] for r in recs], CC.STREAM_CAP, nstates=group[0])
    for r, g in zip(recs, got):
        assert g == r["want"], (r["name"], r["n"], g if isinstance(g, str) else len(g))


@pytest.mark.parametrize("group", GROUPS, ids=[f"{ns}s-L{c}" for ns, c in GROUPS])
def test_streams_device(torch_cuda, group):
    """fsehip_decompress_streams, outputs between guard bands."""
    torch = torch_cuda
    from entropy_coders_amd import load

    nstates, lmax = group
    recs = stream_groups()[group]
    streams = [r["stream"] for r in recs]
    n = len(streams)
    stride = CC.STREAM_CAP
    in_stride = (max(len(x) for x in streams) + 255) // 256 * 256
    host = np.zeros(n * in_stride, dtype=np.uint8)
    for i, x in enumerate(streams):
        host[i * in_stride: i * in_stride + len(x)] = np.frombuffer(x, dtype=np.uint8)
    d_in = torch.from_numpy(host).cuda()
    lens = torch.tensor([len(x) for x in streams], dtype=torch.int32, device="cuda")
    w_out, out = g8(torch, n * stride)
    w_len, out_len = g32(torch, n)
    w_st, status = g32(torch, n)
    rc = load().fsehip_decompress_streams(nstates, lmax, ptr(d_in), in_stride, ptr(lens), n, ptr(out), stride,
                                          ptr(out_len), ptr(status),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert_guards(w_out, out, FILL["uint8"], "out")
    assert_guards(w_len, out_len, FILL["int32"], "out_len")
    assert_guards(w_st, status, FILL["int32"], "status")
    assert_all_written(status, FILL["int32"], "status")
    ho, ol, st = out.cpu().numpy(), out_len.tolist(), status.tolist()
    for i, r in enumerate(recs):
        w = r["want"]
        if isinstance(w, str):
            assert status_name(st[i]) == w, (r["name"], r["n"])
        else:
            assert st[i] == 0 and ol[i] == len(w), (r["name"], r["n"], status_name(st[i]), ol[i], len(w))
            assert ho[i * stride: i * stride + len(w)].tobytes() == w, (r["name"], r["n"])


def decode_block_routes(torch, recs, block, nstates, lmax):
    """The streams as the blocks of one batch (all but the last `block` raw
    bytes long): fsehip_decompress_blocks without a sidecar, then
    fsehip_build_sidecar and the segment route with what it built."""
    from entropy_coders_amd import BlockCodec

    ckpt = 16
    codec = BlockCodec(block_size=block, table_log=lmax if lmax > 11 else 0, ckpt_interval=ckpt, nstates=nstates)
    assert codec.max_table_log == lmax
    nb = len(recs)
    n_total = block * (nb - 1) + recs[-1]["n"]
    assert all(r["n"] == block for r in recs[:-1]) and codec.n_blocks(n_total) == nb
    slot = codec.slot_bytes
    host = np.zeros(nb * slot, dtype=np.uint8)
    for b, r in enumerate(recs):
        assert len(r["stream"]) <= slot
        host[b * slot: b * slot + len(r["stream"])] = np.frombuffer(r["stream"], dtype=np.uint8)
    slots = torch.from_numpy(host).cuda()
    comp_len = torch.tensor([len(r["stream"]) for r in recs], dtype=torch.int32, device="cuda")
    cb = {"n_total": n_total, "out": slots, "comp_len": comp_len}
    what = f"block {block} nstates {nstates} class {lmax} {[r['name'] for r in recs][:3]}"

    def verify(route, w_o, o, w_s, s):
        torch.cuda.synchronize()
        assert_guards(w_o, o, FILL["uint8"], f"{route} out, {what}")
        assert_guards(w_s, s, FILL["int32"], f"{route} status, {what}")
        st, got = s.tolist(), o.cpu().numpy()
        for b, r in enumerate(recs):
            # every written stream's reference decode is its n-byte message (test_caller_cases.test_table_streams)
            assert len(r["want"]) == r["n"]
            assert st[b] == 0, (route, what, b, status_name(st[b]))
            assert got[b * block: b * block + r["n"]].tobytes() == r["want"], (route, what, b, r["name"])

    (w_o, o), (w_s, s) = g8(torch, n_total), g32(torch, nb)
    codec.decompress_into(cb, o, s, use_sidecar=False)
    verify("sidecar-less", w_o, o, w_s, s)

    (w_o, o), (w_s, s) = g8(torch, n_total), g32(torch, nb)
    w_so, side_out = g64(torch, nb * codec.side_per_block)
    side_out.zero_()
    p = codec.params()
    rc = codec.lib.fsehip_build_sidecar(C.byref(p), ptr(slots), slot, ptr(comp_len), ptr(o), n_total, ptr(side_out),
                                        ptr(s), codec._stream())
    if nstates == 1 and lmax > 12:  # 1-state blocks above class 12: refused before anything is written (fsehip.h)
        assert status_name(rc) == "UNSUPPORTED", (what, rc)
        torch.cuda.synchronize()
        assert bool((w_o == FILL["uint8"]).all()) and bool((w_s == FILL["int32"]).all())
        return
    assert rc == 0, (what, rc)
    verify("build_sidecar", w_o, o, w_s, s)
    assert_guards(w_so, side_out, FILL["int64"], f"build_sidecar sidecar_out, {what}")
    cb["sidecar"] = side_out
    (w_o, o), (w_s, s) = g8(torch, n_total), g32(torch, nb)
    codec.decompress_into(cb, o, s, use_sidecar=True)
    verify("segments", w_o, o, w_s, s)


@pytest.mark.parametrize("group", GROUPS, ids=[f"{ns}s-L{c}" for ns, c in GROUPS])
def test_streams_block_routes(torch_cuda, group):
    """The 64-byte messages as one batch of 64-byte blocks; every other
    length as a batch of one block of that size (a batch's blocks are all
    `block_size` long but the last, and block_size is a multiple of 16 in a
    batch of several)."""
    nstates, lmax = group
    recs = stream_groups()[group]
    full = [r for r in recs if r["n"] == 64]
    assert len(full) >= 1
    decode_block_routes(torch_cuda, full, 64, nstates, lmax)
    for r in recs:
        if r["n"] in (2, 3):  # a ragged last block behind two full ones, and alone
            decode_block_routes(torch_cuda, full[:2] + [r], 64, nstates, lmax)
        if r["n"] != 64:
            decode_block_routes(torch_cuda, [r], r["n"], nstates, lmax)


# ---------------------------------------------------------------- 4. histogram_new beyond one counting segment
SEG = 1 << 18  # HIST_SEG: wave_histogram folds its 16-bit sub-counters into counts[] every 2^18 bytes
SEG_LENGTHS = [SEG - 1, SEG, SEG + 1, 2 * SEG + 17]


def seg_content(kind, n):
    rng = np.random.default_rng(0x5E6 + n)
    if kind == "one_value":
        return np.full(n, 0x5A, dtype=np.uint8)
    if kind == "dominant_not_first":  # each segment starts with 7; 200 takes 15 of 16 bytes
        a = np.where(rng.integers(0, 16, n) == 0, rng.integers(0, 256, n), 200).astype(np.uint8)
        a[::SEG] = 7
        return a
    if kind == "dominant_per_segment":
        a = np.empty(n, dtype=np.uint8)
        for k, lo in enumerate(range(0, n, SEG)):
            m = min(SEG, n - lo)
            a[lo: lo + m] = np.where(rng.integers(0, 8, m) == 0, rng.integers(0, 256, m), (31, 144, 250)[k])
        return a
    return rng.integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("kind", ["one_value", "dominant_not_first", "dominant_per_segment", "uniform"])
@pytest.mark.parametrize("n", SEG_LENGTHS)
def test_histogram_new_across_segments(torch_cuda, n, kind):
    from entropy_coders_amd import FseError, histogram_new, norm_histogram_new

    src = seg_content(kind, n)
    want = np.bincount(src, minlength=256)
    h = histogram_new(src)
    assert np.array_equal(np.ctypeslib.as_array(h.counts), want), (n, kind)
    assert h.size == n and h.table_len == int(np.flatnonzero(want)[-1]) + 1

    def ref():
        nh = O.norm_new(src)
        return list(nh.norm), nh.log2, nh.table_len

    def run():
        nh = norm_histogram_new(src)
        return list(nh.norm), nh.log2, nh.table_len

    assert outcome(run, FseError) == outcome(ref, O.OracleError), (n, kind)
