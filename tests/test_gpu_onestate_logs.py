"""The 1-state format (fse_compress / fse_decompress, lib.rs:112-143 / 187-211)
at forced table logs, byte for byte against the oracle.

NormHistogram::new never picks a log above 11, so the 1-state kernels for
tables of 2^12..2^15 entries (encode_blocks_kernel<12..15, 64, 1>, the segment
kernels decode_pre_kernel<12..15, ..., 1>, serial_ring_kernel<12, 3, 1>,
decode1_serial_kernel<13|14|15>) run only when a log is forced.  The expected
bytes are `oracle.compress(src, L)` (fo_compress_log: Histogram::normalize(L)
and the fse_compress body), which the spec model re-derives on the CPU
(tests/test_oracle.py).

At L = 15 new_first_symbol (fse.rs:210-218) panics for most seeds, and the
1-state seed is the last byte alone: the blocks here end in 251, a byte the
generators never produce, whose norm (-1, or a power of two) keeps the index
inside the table; one block of each batch keeps its own last byte and must
carry ENCODER_INIT.  The crate's own decode of an L = 15 stream may differ from
the source in its last symbols, so the expected decode
there is always `oracle.decompress(want)`, n bytes long.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import frame_ref as R
from oracle import oracle as O
from test_gpu_guard_bands import FILL, assert_all_written, assert_guards, g8, g32, g64, ptr

pytestmark = pytest.mark.gpu

LOGS = [5, 8, 11, 12, 13, 14, 15]  # 5, 8, 11: forced below / at the default class; 12..15: one kernel class each
RARE = 251
UNSUPPORTED = -14
KINDS = [(0, 0.77), (2, 0.0), (1, 0.5), (0, 0.155), (2, 0.0), (0, 0.77)]  # skewed, near-uniform, geometric, LUT
# (tail length of the ragged last block, checkpoint interval) per block size:
# 2 and 3 bytes, an odd and an even length.  At L = 15 the longer tails keep
# the rare byte's norm at 8 (block 4096: 32768 / n rounds down to 8) or -1
# (block 65536: n >= 32768).
TAILS = {4096: [(2, 64), (3, 128), (3763, 128), (3900, 64)], 65536: [(2, 64), (3, 128), (65203, 128), (40000, 64)]}


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


def eff_log(comp):
    return (comp[0] & 15) + 5


# ---------------------------------------------------------------- the shared reference (computed once, read-only)
@functools.lru_cache(maxsize=None)
def full_block(L, block, i):
    """Full block i of the (L, block) data set with the oracle's result: (raw,
    (bytes, payload bits) or a status name, the crate's decode or None).  At
    L = 15 every block but number 2 ends in the rare byte."""
    kind, prob = KINDS[i]
    raw = O.generate(kind, prob, 0x5EED0400 + L, i, block)
    if L == 15 and i != 2:
        raw[-1] = RARE
    raw.setflags(write=False)
    return (raw,) + reference(raw, L)


def reference(raw, L):
    try:
        want = O.compress(raw, L)
    except O.OracleError as e:
        return e.code, None
    if len(set(raw.tolist())) == 1:
        return want, None
    dec = O.decompress(want[0])
    assert len(dec) == len(raw), (L, len(raw), len(dec))  # the crate's decoder stops after n symbols at every log
    if eff_log(want[0]) < 15:
        assert dec == raw.tobytes(), (L, len(raw))
    return want, np.frombuffer(dec, np.uint8)


@functools.lru_cache(maxsize=None)
def tail_block(L, tail):
    if tail <= 3:
        raw = np.array([7, 3, 7][:tail], np.uint8)
        if L == 15 and tail == 2:
            raw[-1] = RARE  # two symbols of norm 2^14; three bytes cannot encode at 15: that tail is the unpatched block
    else:
        raw = O.generate(0, 0.155, 0x5EED0500 + L, tail, tail)
        if L == 15:
            raw[-1] = RARE
    raw.setflags(write=False)
    return (raw,) + reference(raw, L)


def batch_of(L, block, tail):
    """6 full blocks and the ragged tail.  At L = 15 with the 3-byte tail every
    full block is patched (the tail is the unpatched one)."""
    blocks = [full_block(L, block, i) for i in range(len(KINDS))]
    if L == 15 and tail == 3:
        raw = np.array(blocks[2][0])
        raw[-1] = RARE
        blocks[2] = (raw,) + reference(raw, L)
    return blocks + [tail_block(L, tail)]


# ---------------------------------------------------------------- a, b: the batch encoder and every decode route
def check_batch(torch, L, block, tail, ckpt):
    from entropy_coders_amd import BlockCodec

    blocks = batch_of(L, block, tail)
    nb = len(blocks)
    what = f"L {L} block {block} tail {tail} ckpt {ckpt}"
    host = np.concatenate([b[0] for b in blocks])
    n_total = len(host)
    codec = BlockCodec(block_size=block, table_log=L, ckpt_interval=ckpt, nstates=1)
    assert codec.n_blocks(n_total) == nb and codec.max_table_log == max(L, 11)
    failed = [b for b in range(nb) if isinstance(blocks[b][1], str)]
    if L == 15:  # exactly the unpatched block is the reference's panic; the oracle accepts every patched one
        assert failed == [nb - 1 if tail == 3 else 2], (what, [blocks[b][1] for b in failed])
        assert blocks[failed[0]][1] == "ENCODER_INIT" and blocks[failed[0]][0][-1] != RARE
        assert all(blocks[b][0][-1] == RARE for b in range(nb) if b not in failed)
    else:
        assert failed == [], (what, failed)
    src = torch.from_numpy(host).cuda()
    u8, i32, i64 = FILL["uint8"], FILL["int32"], FILL["int64"]
    spb = codec.side_per_block

    # ---- encode into guarded arrays: bytes, payload bits, status, sidecar
    w_out, out = g8(torch, nb * codec.slot_bytes)
    w_len, comp_len = g32(torch, nb)
    w_bits, bits = g32(torch, nb)
    w_st, status = g32(torch, nb)
    w_side, side = g64(torch, nb * spb)
    side.zero_()  # as BlockCodec.alloc: entries past a block's checkpoints stay zero
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
    est = status.tolist()
    hside = side.cpu().numpy().view(np.uint64)
    for b, (raw, want, _) in enumerate(blocks):
        if isinstance(want, str):
            assert status_name(est[b]) == want, (what, b, est[b])
            assert int(comp_len[b]) == 0, (what, b)
            continue
        assert est[b] == 0, (what, b, status_name(est[b]))
        assert codec.block_bytes(cb, b) == want[0], (what, b)
        assert int(bits[b]) == want[1], (what, b)
        assert eff_log(want[0]) <= codec.max_table_log
        bp, s0 = O.checkpoints1(want[0], ckpt)
        assert len(bp) == (len(raw) - 1) // ckpt + 1 <= spb, (what, b)
        mine = hside[b * spb: b * spb + len(bp)]
        assert np.array_equal(mine & np.uint64(0xFFFFFFFF), bp.astype(np.uint64)), f"sidecar bit positions, {what} block {b}"
        assert np.array_equal(mine >> np.uint64(32), s0.astype(np.uint64)), f"sidecar states, {what} block {b}"

    # ---- decode, every route
    ok = [b for b in range(nb) if b not in failed]

    def fresh():
        return g8(torch, n_total), g32(torch, nb)

    def verify(route, w_o, o, w_s, s):
        torch.cuda.synchronize()
        assert_guards(w_o, o, u8, f"{route} out, {what}")
        assert_guards(w_s, s, i32, f"{route} status, {what}")
        st = s.tolist()
        got = o.cpu().numpy()
        for b, (raw, want, dec) in enumerate(blocks):
            if b in failed:  # nothing was encoded: the decoder's status for an empty stream
                assert status_name(st[b]) == "EMPTY", (route, what, b, st[b])
                continue
            assert st[b] == 0, (route, what, b, status_name(st[b]))
            if dec is not None:
                assert np.array_equal(got[b * block: b * block + len(raw)], dec), (route, what, b)

    for use_sidecar in (True, False):
        (w_o, o), (w_s, s) = fresh()
        codec.decompress_into(cb, o, s, use_sidecar=use_sidecar)
        verify("sidecar segments" if use_sidecar else "sidecar-less serial", w_o, o, w_s, s)

    # prebuilt tables: entry by entry against the oracle's DecodeTable, then both decodes with them
    p = codec.params()
    per = int(codec.lib.fsehip_dtable_bytes(codec.max_table_log))
    w_dt, dt = g32(torch, nb * per // 4)
    w_info, info = g32(torch, nb)
    rc = codec.lib.fsehip_build_dtables(C.byref(p), ptr(out), codec.slot_bytes, ptr(comp_len), nb, ptr(dt), ptr(info),
                                        codec._stream())
    assert rc == 0, (what, rc)
    torch.cuda.synchronize()
    assert_guards(w_dt, dt, i32, f"build_dtables tables, {what}")
    assert_guards(w_info, info, i32, f"build_dtables info, {what}")
    hinfo = info.tolist()
    hdt = dt.cpu().numpy().view(np.uint32)
    sh = 17 if codec.max_table_log >= 15 else 18  # newState field (fsehip.h, fsehip_build_dtables)
    for b in ok:
        tl, ns, sym, nbits, used = O.dtable(blocks[b][1][0])
        assert hinfo[b] >> 16 == tl and hinfo[b] & 0xFFFF == used, (what, b, hinfo[b])
        e = hdt[b * (per // 4): b * (per // 4) + (1 << tl)]
        assert np.array_equal(e & 0xFF, nbits), (what, b)
        assert np.array_equal((e >> 8) & 0xFF, sym), (what, b)
        assert np.array_equal(e >> sh, ns), (what, b)
    for b in failed:
        assert status_name(hinfo[b]) == "EMPTY", (what, b, hinfo[b])
    for use_sidecar in (True, False):
        (w_o, o), (w_s, s) = fresh()
        codec.decompress_dt_into(cb, {"dt": dt, "info": info}, o, s, use_sidecar=use_sidecar)
        verify(f"prebuilt tables, sidecar {use_sidecar}", w_o, o, w_s, s)
    assert_guards(w_dt, dt, i32, f"decompress_blocks_dt tables, {what}")

    # fsehip_build_sidecar: the encoder's sidecar up to class 12, UNSUPPORTED (and nothing written) above
    (w_o, o), (w_s, s) = fresh()
    w_so, side_out = g64(torch, nb * spb)
    rc = codec.lib.fsehip_build_sidecar(C.byref(p), ptr(out), codec.slot_bytes, ptr(comp_len), ptr(o), n_total,
                                        ptr(side_out), ptr(s), codec._stream())
    if codec.max_table_log <= 12:
        assert rc == 0, (what, rc)
        verify("build_sidecar", w_o, o, w_s, s)
        assert_guards(w_so, side_out, i64, f"build_sidecar sidecar_out, {what}")
        rebuilt = side_out.cpu().numpy().view(np.uint64)
        for b in ok:
            k = (len(blocks[b][0]) - 1) // ckpt + 1
            assert np.array_equal(rebuilt[b * spb: b * spb + k], hside[b * spb: b * spb + k]), (what, b)
    else:
        assert rc == UNSUPPORTED, (what, rc)
        torch.cuda.synchronize()
        for w, f, name in ((w_o, u8, "out"), (w_s, i32, "status"), (w_so, i64, "sidecar_out")):
            assert bool((w == f).all()), f"build_sidecar wrote {name} before returning UNSUPPORTED, {what}"


@pytest.mark.parametrize("tail_i", range(4), ids=["tail2", "tail3", "odd", "even"])
@pytest.mark.parametrize("block", [4096, 65536])
@pytest.mark.parametrize("L", LOGS)
def test_batch_encode_and_decode_routes(torch_cuda, L, block, tail_i):
    tail, ckpt = TAILS[block][tail_i]
    check_batch(torch_cuda, L, block, tail, ckpt)


@pytest.mark.parametrize("L", [12, 13, 14])
def test_blocks_on_both_sides_of_the_stage(L):
    """The 64 KiB data set puts blocks below the first stage (36 KiB at L = 12,
    44 KiB at 13 and 14) and above it (the near-uniform ones: the list pass),
    so test_batch_encode_and_decode_routes runs both passes.  Oracle only."""
    lens = [len(full_block(L, 65536, i)[1][0]) for i in range(len(KINDS))]
    assert min(lens) < 36 * 1024 and max(lens) > 44 * 1024, lens
    assert sum(ln > 44 * 1024 for ln in lens) >= 2 and sum(ln < 36 * 1024 for ln in lens) >= 2, lens


# ---------------------------------------------------------------- c: fsehip_compress_streams
STREAM_LENGTHS = [2, 3, 17, 4096, 65536]


@functools.lru_cache(maxsize=None)
def stream_source(L, n):
    raw = np.array([7, 3, 7][:n], np.uint8) if n <= 3 else O.generate(0, 0.155, 0x5EED0600 + L, n, n)
    if L == 15:
        raw[-1] = RARE
    raw.setflags(write=False)
    return (raw,) + reference(raw, L)


@pytest.mark.parametrize("L", LOGS)
def test_compress_streams_forced_log(torch_cuda, L):
    """Each length three times in one call: a worst-case region, a region of
    exactly the compressed length, and one a byte short of it (DST_TOO_SMALL,
    the filler after the region untouched).  Streams the oracle rejects (at
    L = 15: 3 and 17 bytes, whose seed has a norm that is no power of two) carry
    its status in all three."""
    from entropy_coders_amd import compress_streams, load

    lib = load()
    lmax = max(L, 11)
    srcs = [stream_source(L, n) for n in STREAM_LENGTHS]
    if L == 15:
        assert [isinstance(w, str) for _, w, _ in srcs] == [False, True, True, False, False], [w for _, w, _ in srcs]
    else:
        assert not any(isinstance(w, str) for _, w, _ in srcs)
    bufs, caps, expect = [], [], []
    for raw, want, _ in srcs:
        worst = int(lib.fsehip_stream_out_bytes(len(raw), lmax))
        for variant in ("worst", "exact", "short"):
            bufs.append(raw)
            if isinstance(want, str):
                caps.append(worst)
                expect.append(want)
            elif variant == "short":
                caps.append(len(want[0]) - 1)
                expect.append("DST_TOO_SMALL")
            else:
                caps.append(worst if variant == "worst" else len(want[0]))
                expect.append(want)
    st, cl, pb, ho, desc = compress_streams(bufs, nstates=1, table_log=L, out_caps=caps, raw=True)
    canary = np.ones(len(ho), bool)
    for i, ((_, off, n, cap), want) in enumerate(zip(desc, expect)):
        canary[off: off + cap] = False
        if isinstance(want, str):
            assert status_name(st[i]) == want and cl[i] == 0, (L, i, n, cap, status_name(st[i]), want)
            continue
        assert st[i] == 0, (L, i, n, cap, status_name(st[i]))
        assert ho[off: off + int(cl[i])].tobytes() == want[0], (L, i, n, cap)
        assert int(pb[i]) & 0xFFFFFFFF == want[1], (L, i, n)
    assert bool((ho[canary] == 0xA5).all()), f"L {L}: a store outside a stream's region"
    if L >= 12:  # a kernel class below the forced log
        got = compress_streams([s[0] for s in srcs], nstates=1, table_log=L, max_table_log=L - 1)
        assert got == ["UNSUPPORTED"] * len(srcs), (L, got)


# ---------------------------------------------------------------- d: the reference-mode decoders on oracle streams
STRIDE = 4096


@functools.lru_cache(maxsize=None)
def crate_streams():
    """33 oracle streams, three at each table log 5..15, of raw lengths below,
    at and above STRIDE; every 7th is damaged (a flipped byte and a one-byte
    truncation in turn).  Returns (streams, header logs, the oracle's
    reference-mode result within STRIDE bytes: bytes or a status name)."""
    rng = np.random.default_rng(0x1057)
    streams = []
    for L in range(5, 16):
        for j, n in enumerate((1024, 4096, 8192) if L == 15 else (1001, 4096, 8191)):
            kind, prob = [(0, 0.155), (0, 0.77), (2, 0.0), (1, 0.5)][(L + j) % 4]
            raw = O.generate(kind, prob, 0x5EED0700 + L, j, n)
            if L == 15:
                raw[-1] = RARE  # norm 32, 8 and 4: powers of two
            comp = bytearray(O.compress(raw, L)[0])  # a rejected source fails the test here
            assert eff_log(comp) >= L
            i = len(streams)
            if i % 7 == 6:
                if (i // 7) % 2:
                    del comp[-1]
                else:
                    comp[int(rng.integers(0, len(comp)))] ^= 0x5A
            streams.append(bytes(comp))
    logs = [eff_log(x) for x in streams]
    assert sum(v <= 11 for v in logs) >= 3 and logs.count(12) >= 3 and sum(v >= 13 for v in logs) >= 3
    assert {13, 14, 15} <= set(logs)
    want = []
    for x in streams:
        try:
            want.append(O.decompress(x, STRIDE))
        except O.OracleError as e:
            want.append(e.code)
    good = [w for w in want if not isinstance(w, str)]
    assert any(len(w) < STRIDE for w in good) and any(len(w) == STRIDE for w in good) and "DST_TOO_SMALL" in want
    return streams, logs, want


@pytest.mark.parametrize("bound", [11, 12, 13, 14, 15])
def test_decompress_streams_bounds(torch_cuda, bound):
    """fsehip_decompress_streams(nstates = 1) at each kernel bound, outputs
    between guard bands: UNSUPPORTED above the bound, the oracle's bytes or
    status below it."""
    torch = torch_cuda
    from entropy_coders_amd import load

    streams, logs, want = crate_streams()
    n = len(streams)
    in_stride = (max(len(x) for x in streams) + 255) // 256 * 256
    host = np.zeros(n * in_stride, dtype=np.uint8)
    for i, x in enumerate(streams):
        host[i * in_stride: i * in_stride + len(x)] = np.frombuffer(x, dtype=np.uint8)
    d_in = torch.from_numpy(host).cuda()
    lens = torch.tensor([len(x) for x in streams], dtype=torch.int32, device="cuda")
    w_out, out = g8(torch, n * STRIDE)
    w_len, out_len = g32(torch, n)
    w_st, status = g32(torch, n)
    rc = load().fsehip_decompress_streams(1, bound, ptr(d_in), in_stride, ptr(lens), n, ptr(out), STRIDE, ptr(out_len),
                                          ptr(status), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert_guards(w_out, out, FILL["uint8"], "out")
    assert_guards(w_len, out_len, FILL["int32"], "out_len")
    assert_guards(w_st, status, FILL["int32"], "status")
    assert_all_written(status, FILL["int32"], "status")
    ho, ol, st = out.cpu().numpy(), out_len.tolist(), status.tolist()
    for i, w in enumerate(want):
        if logs[i] > bound:
            assert status_name(st[i]) == "UNSUPPORTED", (bound, i, logs[i], status_name(st[i]))
        elif isinstance(w, str):
            assert status_name(st[i]) == w, (bound, i, logs[i], w, status_name(st[i]))
        else:
            assert st[i] == 0 and ol[i] == len(w), (bound, i, logs[i], status_name(st[i]), ol[i], len(w))
            assert ho[i * STRIDE: i * STRIDE + len(w)].tobytes() == w, (bound, i, logs[i])


def test_decompress_many_mixed_logs(torch_cuda):
    """fse_decompress_many: all three groups (header log <= 11, 12, 13..15) in
    one call, and a call of two streams (the single-stream path)."""
    from entropy_coders_amd import decompress2_many

    streams, logs, want = crate_streams()
    assert decompress2_many(streams, STRIDE, nstates=1) == want
    pair = [logs.index(13), logs.index(15) + 1]
    assert decompress2_many([streams[i] for i in pair], STRIDE, nstates=1) == [want[i] for i in pair]


def test_host_decompress_each_log(torch_cuda):
    """The lone fse_decompress on each stream (single_decode_kernel up to 11,
    the serial kernels above)."""
    from entropy_coders_amd import FseError, decompress

    streams, logs, want = crate_streams()
    for i, (x, w) in enumerate(zip(streams, want)):
        if isinstance(w, str):
            with pytest.raises(FseError) as e:
                decompress(x, cap=STRIDE)
            assert e.value.code == w, (i, logs[i], w, e.value.code)
        else:
            assert decompress(x, cap=STRIDE) == w, (i, logs[i])


# ---------------------------------------------------------------- e: the frame
@pytest.mark.parametrize("table_log", [12, 13])
def test_frame_onestate_forced_log(torch_cuda, table_log):
    """A 1-state frame at a forced log, 3 blocks per chunk: the bytes of
    frame_ref (oracle blocks, the device's sidecars), the round trip, and one
    unaligned range across a block boundary."""
    torch = torch_cuda
    from entropy_coders_amd import BlockCodec

    raw = R.corpus(1000)
    codec = BlockCodec(block_size=R.BLOCK, table_log=table_log, ckpt_interval=R.CKPT, nstates=1)
    src = torch.from_numpy(raw).cuda()
    cb = codec.compress(src)
    side = cb["sidecar"].cpu().numpy().view(np.uint64)
    frame = codec.compress_frame(src, chunk_blocks=3)
    want = R.build_frame(raw, R.BLOCK, R.CKPT, 1, table_log, sidecars=side)
    got = frame.cpu().numpy().tobytes()
    assert len(got) == len(want) and got == want
    assert R.types_of(got)[:2] == [R.FSE, R.FSE] and R.decode_frame(got) == raw.tobytes()
    info = codec.frame_info(frame)
    assert (info.nstates, info.max_table_log, info.n_total) == (1, table_log, len(raw))
    out, st = BlockCodec().decompress_frame(frame, chunk_blocks=3)  # the frame alone decides
    assert not bool(st.any()) and out.cpu().numpy().tobytes() == raw.tobytes()
    lo, ln = R.BLOCK - 77, 301  # from block 0 into block 1, both FSE
    part = codec.decompress_frame_range(frame, lo, ln, chunk_blocks=3)
    assert part.cpu().numpy().tobytes() == raw[lo: lo + ln].tobytes()
