"""Shared-table coding on the GPU (include/fsehip.h section 2c): exact
payloads, bit counts and statuses against tests/shared_ref.py (which
tests/test_shared_table_ref.py pins to the C oracle), the own-table pin to the
oracle's streams, both decode modes, statuses that stay with their message,
where the calls write, and stream order."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import shared_ref as R
from entropy_coders_amd import _lib
from oracle import oracle as O
from oracle.spec import SpecError
from test_gpu_guard_bands import FILL, assert_guards, g8, g32, ptr

pytestmark = pytest.mark.gpu

A5, F32 = FILL["uint8"], FILL["int32"]
LENGTHS = [2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 4096, 4099, 65535, 65536]
ALPHA = np.array([3, 9, 27, 81, 128, 200, 255], dtype=np.uint8)
SMALL = [0, 6, 13, 4, 1, 2]  # symbols of the L = 5 table below, by weight


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module", autouse=True)
def rank_fallbacks_stay_zero(torch_cuda):
    """No table of this file's calls fell back to the peer-mask ranks."""
    lib = _lib.load()
    c = (C.c_uint32 * 3)()
    assert lib.fsehip_rank_fallbacks(0, C.byref(c), 1) == 0  # read and reset
    yield
    assert lib.fsehip_rank_fallbacks(0, C.byref(c), 0) == 0
    assert list(c) == [0, 0, 0]


# ---------------------------------------------------------------- tables and messages (host)
def _l5_table():
    t = [0] * 256
    for s, v in zip(SMALL, (13, 9, 6, -1, -1, 2)):
        t[s] = v
    return R.try_from(t)


@lru_cache(maxsize=None)
def tables():
    """name -> (norm, table log, table_len); computed at first use."""
    sample = O.generate(0, 0.155, 0x5EED0B00, 0, 65536).tobytes()
    seven = ALPHA[np.random.default_rng(0x7AB1E).integers(0, 7, 4096)].tobytes()
    counts = [0] * 256
    for b in seven:
        counts[b] += 1
    t = {"trained-11": R.train([sample], 11, 1), "trained-12": R.train([sample], 12, 1),
         "seven-9": spec_normalize(counts, len(seven), 9), "L5": _l5_table()}
    assert list(t) == TABLE_NAMES and [v[1] for v in t.values()] == [11, 12, 9, 5]
    assert t["L5"][2] == 14 and t["seven-9"][2] == 256
    return t


def spec_normalize(counts, size, L):
    from oracle import spec

    tl = max(i for i in range(256) if counts[i]) + 1
    norm, log2, _ = spec.normalize(counts, size, tl, L)
    return norm, log2, tl


TABLE_NAMES = ["trained-11", "trained-12", "seven-9", "L5"]


def data(name, n, seed):
    """n bytes every one of which has a slot in table `name`."""
    if name.startswith("trained"):
        return O.generate(0, 0.155, 0x5EED0B01, seed, n).tobytes()
    rng = np.random.default_rng(seed)
    if name == "seven-9":
        return ALPHA[rng.integers(0, 7, n)].tobytes()
    return np.array(SMALL, dtype=np.uint8)[rng.choice(6, n, p=[13 / 32, 9 / 32, 6 / 32, 1 / 32, 1 / 32, 2 / 32])].tobytes()


_REF = {}


def ref(name, m, nstates):
    """shared_ref's (payload, bits) or status name, computed once per message."""
    key = (name, nstates, m)
    if key not in _REF:
        try:
            _REF[key] = R.compress_shared(m, *tables()[name], nstates)
        except SpecError as e:
            _REF[key] = e.code
    return _REF[key]


def messages(name, nstates, count=300):
    """`count` messages whose lengths cycle through LENGTHS (with 1 at one
    state).  The reference is pure Python, so messages from 1,000 bytes on come
    in two variants per length and the two longest in one."""
    lens = LENGTHS + ([1] if nstates == 1 else [])
    out = []
    for i in range(count):
        n = lens[i % len(lens)]
        variant = i if n < 1000 else (i // len(lens)) % 2 if n < 65535 else 0
        out.append(data(name, n, 1000 * variant + n % 997))
    return out


def nh_of(norm, L, tl):
    nh = _lib.NormHistogram()
    for s in range(256):
        nh.norm[s] = norm[s]
    nh.log2, nh.table_len = L, tl
    return nh


@pytest.fixture(scope="module")
def shared(torch_cuda):
    from entropy_coders_amd import SharedTable

    return {k: SharedTable(nh_of(*t)) for k, t in tables().items()}


# ---------------------------------------------------------------- 1. exact bytes, bits and statuses
@pytest.mark.parametrize("nstates", [2, 1])
@pytest.mark.parametrize("name", TABLE_NAMES)
def test_exact_payloads(shared, name, nstates):
    msgs = messages(name, nstates)
    want = [ref(name, m, nstates) for m in msgs]
    assert not any(isinstance(w, str) for w in want)
    for count in (300, 1, 257):  # two workgroups, one lane, one lane of a second workgroup
        got = shared[name].compress(msgs[:count], nstates=nstates)
        assert len(got) == count
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (name, nstates, count, i, len(msgs[i]), g if isinstance(g, str) else (len(g[0]), g[1]),
                            (len(w[0]), w[1]))


# ---------------------------------------------------------------- 2. the own-table pin
OWN = [(2, 9), (3, 11), (5, 12), (17, 9), (64, 11), (255, 12), (300, 9), (1024, 11), (4096, 12), (4097, 11)]


def own_message(n, L):
    """The skewed generator from 64 bytes on; below, 7 symbols of which two at least occur."""
    return data("trained", n, 77 * L + n) if n >= 64 else (ALPHA[:2].tobytes() + data("seven-9", n, 77 * L + n))[:n]


@pytest.mark.parametrize("nstates", [2, 1])
def test_own_table_payload_is_the_oracles_stream(torch_cuda, nstates):
    from entropy_coders_amd import SharedTable

    for n, L in OWN:
        m = own_message(n, L)
        stream, bits = O.compress2(m, L) if nstates == 2 else O.compress(m, L)
        _, used = O.header_read(stream)
        nh, _ = O.normalize(O.hist_count(m), L)
        table = SharedTable(nh_of(list(nh.norm), nh.log2, nh.table_len))
        assert table.compress([m], nstates=nstates) == [(stream[used:], bits)], (n, L)
        # and back, the table taken from the stream's header
        hdr, used2 = O.header_read(stream)
        assert used2 == used
        table = SharedTable(nh_of(list(hdr.norm), hdr.log2, hdr.table_len))
        assert table.decompress([stream[used:]], raw_lens=[len(m)], nstates=nstates) == [m], (n, L)
        # without the length: where the crate's decoder ends (a short message whose table has a symbol above
        # half of it has steps that cost no bit, and the crate reads on: the oracle says how far)
        try:
            crate = (O.decompress2 if nstates == 2 else O.decompress)(stream, len(m) + 5)
        except O.OracleError as e:
            crate = e.code
        assert table.decompress([stream[used:]], nstates=nstates, out_cap=len(m) + 5) == [crate], (n, L)
        assert crate == m or n < 64, (n, L)


# ---------------------------------------------------------------- 3. decode
@pytest.mark.parametrize("nstates", [2, 1])
@pytest.mark.parametrize("name", ["trained-11", "seven-9", "L5"])
def test_round_trip_both_modes(shared, name, nstates):
    msgs = messages(name, nstates)
    payloads = [p for p, _ in shared[name].compress(msgs, nstates=nstates)]
    assert shared[name].decompress(payloads, raw_lens=[len(m) for m in msgs], nstates=nstates) == msgs
    # no lengths: the crate's own end, in regions with a few bytes to spare or none
    caps = [len(m) + (i % 3) * 7 for i, m in enumerate(msgs)]
    assert shared[name].decompress(payloads, nstates=nstates, out_cap=caps) == msgs


def test_single_symbol_table(torch_cuda):
    from entropy_coders_amd import SharedTable

    t = [0] * 256
    t[65] = 1 << 9
    norm, L, tl = R.try_from(t)
    table = SharedTable(nh_of(norm, L, tl))
    for nstates in (2, 1):
        msgs = [b"A" * n for n in (2, 3, 37, 64, 1000)] + ([b"A"] if nstates == 1 else [])
        got = table.compress(msgs, nstates=nstates)
        assert got == [R.compress_shared(m, norm, L, tl, nstates) for m in msgs]
        assert all(bits == nstates * L + 1 for _, bits in got)  # every step costs no bit
        payloads = [p for p, _ in got]
        assert table.decompress(payloads, raw_lens=[len(m) for m in msgs], nstates=nstates) == msgs
        assert table.decompress(payloads, nstates=nstates) == ["SINGLE_SYMBOL"] * len(msgs)
    assert table.compress([b"AAB"]) == ["SYMBOL_NOT_IN_TABLE"]


# ---------------------------------------------------------------- the calls themselves, between guards
def device_call(torch, kind, table, nstates, descs, host_in, out_bytes, raw_lens=None):
    """One fsehip_compress_shared / fsehip_decompress_shared call on guarded
    arrays: (statuses, lengths, payload bits or None, out bytes).  The output
    starts as 0xA5 everywhere; guards of every array are checked."""
    lib = _lib.load()
    n = len(descs)
    desc = (_lib.StreamDesc * n)(*[_lib.StreamDesc(*d) for d in descs])
    d_in = torch.from_numpy(np.frombuffer(bytes(host_in), dtype=np.uint8).copy()).cuda()
    d_desc = torch.from_numpy(np.frombuffer(bytes(desc), dtype=np.uint8).copy()).cuda()
    w_out, out = g8(torch, out_bytes)
    w_len, lens = g32(torch, n)
    w_st, status = g32(torch, n)
    hs = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if kind == "compress":
        w_bits, bits = g32(torch, n)
        rc = lib.fsehip_compress_shared(nstates, ptr(table.image), ptr(d_in), ptr(d_desc), n, ptr(out), ptr(lens),
                                        ptr(bits), ptr(status), hs)
    else:
        w_bits = bits = None
        d_raw = None if raw_lens is None else torch.tensor(list(raw_lens), dtype=torch.int32, device="cuda")
        rc = lib.fsehip_decompress_shared(nstates, ptr(table.image), ptr(d_in), ptr(d_desc), n, ptr(out),
                                          ptr(d_raw) if d_raw is not None else None, ptr(lens), ptr(status), hs)
    assert rc == 0, _lib.STATUS.get(rc, rc)
    torch.cuda.synchronize()
    assert_guards(w_out, out, A5, f"{kind} d_out")
    assert_guards(w_len, lens, F32, f"{kind} lengths")
    assert_guards(w_st, status, F32, f"{kind} d_status")
    if bits is not None:
        assert_guards(w_bits, bits, F32, "d_payload_bits")
        assert not bool((bits == F32).any())
    assert not bool((lens == F32).any()) and not bool((status == F32).any()), "an element was never written"
    return ([_lib.STATUS[s] for s in status.tolist()], lens.tolist(), bits.tolist() if bits is not None else None,
            out.cpu().numpy())


def layout(lengths, caps, gap=64):
    """Descriptors: inputs back to back at 16-byte offsets, regions `gap` bytes apart."""
    descs, so, oo = [], 0, 0
    for n, cap in zip(lengths, caps):
        descs.append((so, oo, n, cap))
        so += (n + 15) // 16 * 16
        oo += (cap + 15) // 16 * 16 + gap
    return descs, max(so, 16), oo


def pack(descs, bufs, size):
    host = np.zeros(size, dtype=np.uint8)
    for (so, _, n, _), b in zip(descs, bufs):
        host[so: so + n] = np.frombuffer(b, dtype=np.uint8)
    return host


def assert_gaps(out, descs, what):
    """Every byte outside the regions still holds 0xA5."""
    inside = np.zeros(len(out), dtype=bool)
    for _, oo, _, cap in descs:
        inside[oo: oo + cap] = True
    assert bool((out[~inside] == A5).all()), f"{what}: a store outside the output regions"


# ---------------------------------------------------------------- 4. statuses isolate
@pytest.mark.parametrize("nstates", [2, 1])
def test_compress_statuses_isolate(torch_cuda, shared, nstates):
    torch = torch_cuda
    good = [data("seven-9", n, 50 + n) for n in (300, 17, 64, 1000, 33, 255, 4096, 31, 2)]
    bad = {1: (good[0][:100] + b"\x04" + good[0][100:], "SYMBOL_NOT_IN_TABLE"),   # a byte whose count is 0
           3: (b"", "EMPTY"), 5: (ALPHA[:1].tobytes(), "TOO_SHORT" if nstates == 2 else None),
           7: (data("seven-9", 65537, 1), "UNSUPPORTED"), 9: (good[1], "DST_TOO_SMALL"), 11: (good[1], None),
           13: (good[2], "BAD_ARG"), 15: (good[3][:-1] + b"\x00", "SYMBOL_NOT_IN_TABLE")}  # ... in the first byte walked
    msgs, want = [], []
    for i in range(17):
        m, status = bad[i] if i in bad else (good[i // 2], None)
        msgs.append(m)
        want.append(status or ref("seven-9", m, nstates))
    L = tables()["seven-9"][1]
    caps = [int(_lib.load().fsehip_shared_out_bytes(len(m), L)) for m in msgs]
    caps[9] = len(ref("seven-9", good[1], nstates)[0]) - 1   # one byte short
    caps[11] = caps[9] + 1                                    # exactly the payload
    descs, in_size, out_size = layout([len(m) for m in msgs], caps)
    descs[13] = (descs[13][0], descs[13][1] + 8, descs[13][2], descs[13][3] - 8)  # out_off no multiple of 16
    st, cl, pb, out = device_call(torch, "compress", shared["seven-9"], nstates, descs, pack(descs, msgs, in_size),
                                  out_size)
    assert_gaps(out, descs, "compress")
    for i, w in enumerate(want):
        if isinstance(w, str):
            assert (st[i], cl[i], pb[i]) == (w, 0, 0), (i, st[i], cl[i], w)
        else:
            assert (st[i], cl[i], pb[i]) == ("OK", len(w[0]), w[1]), (i, st[i], cl[i], pb[i])
            assert out[descs[i][1]: descs[i][1] + cl[i]].tobytes() == w[0], i
    # a byte at or past table_len
    small = [data("L5", 40, 1), data("L5", 40, 2)[:20] + bytes([14]) + data("L5", 40, 2)[20:], data("L5", 40, 3),
             data("L5", 9, 4) + bytes([200])]
    assert shared["L5"].compress(small, nstates=nstates) == [ref("L5", small[0], nstates), "SYMBOL_NOT_IN_TABLE",
                                                            ref("L5", small[2], nstates), "SYMBOL_NOT_IN_TABLE"]


def test_failed_builds(torch_cuda):
    from entropy_coders_amd import FseError, SharedTable

    norm, L, tl = tables()["trained-11"]
    off = list(norm)
    off[0] += 1  # the counts no longer sum to 2^L
    m = data("trained-11", 100, 5)
    for nh, want in ((nh_of(off, L, tl), "BAD_TABLE"), (nh_of(norm, 13, tl), "UNSUPPORTED"),
                     (nh_of(norm, 4, tl), "TABLELOG_RANGE"), (nh_of(norm, L, 0), "BAD_TABLE")):
        assert want == R.build_status(list(nh.norm), nh.log2, nh.table_len)
        table = SharedTable(nh, check_build=False)
        assert table.status == want
        for nstates in (2, 1):
            assert table.compress([m, b"", m[:1], m], nstates=nstates) == ["BAD_TABLE"] * 4
            assert table.decompress([m, b"", m[:1]], nstates=nstates, out_cap=64) == ["BAD_TABLE"] * 3
        with pytest.raises(FseError) as e:
            SharedTable(nh)
        assert e.value.code == want


@pytest.mark.parametrize("nstates", [2, 1])
def test_decompress_statuses_isolate(torch_cuda, shared, nstates):
    torch = torch_cuda
    name = "trained-11"
    norm, L, tl = tables()[name]
    msgs = [data(name, n, 90 + n) for n in (300, 64, 1000, 17)]
    pay = [ref(name, m, nstates)[0] for m in msgs]
    # (payload, raw_len or None, out_cap, expected status or the message)
    rows = [(pay[0], 300, 300, msgs[0]), (pay[0][:-1] + b"\0", 300, 300, "NO_MARKER"), (pay[1], 64, 64, msgs[1]),
            (b"\x01", 5, 16, "TOO_SHORT"), (pay[2], 1000, 1000, msgs[2]), (pay[0], 299, 300, "LENGTH_MISMATCH"),
            (pay[3], 17, 32, msgs[3]), (pay[0], 301, 304, "LENGTH_MISMATCH"), (pay[1], 64, 80, msgs[1]),
            (b"", 5, 16, "EMPTY"), (pay[2], 1000, 999, "DST_TOO_SMALL"), (pay[3], 17, 17, msgs[3])]
    for known in (True, False):
        use = [r for r in rows if known or r[3] not in ("LENGTH_MISMATCH",)]
        if not known:  # the crate's own end within out_cap: one byte short is DST_TOO_SMALL
            use = [(p, None, cap, w) for p, _, cap, w in use] + [(pay[0], None, 299, "DST_TOO_SMALL"),
                                                                 (pay[1], None, 64, msgs[1])]
        for p, raw, cap, w in use:  # the table of expectations against the reference first
            try:
                r = R.decompress_shared(p, norm, L, tl, nstates, raw_len=raw, out_cap=cap)
            except SpecError as e:
                r = e.code
            assert r == w, (known, len(p), raw, cap, r if isinstance(r, str) else len(r))
        descs, in_size, out_size = layout([len(r[0]) for r in use], [r[2] for r in use])
        st, ol, _, out = device_call(torch, "decompress", shared[name], nstates, descs,
                                     pack(descs, [r[0] for r in use], in_size), out_size,
                                     [r[1] for r in use] if known else None)
        assert_gaps(out, descs, "decompress")
        for i, (_, _, _, w) in enumerate(use):
            if isinstance(w, str):
                assert (st[i], ol[i]) == (w, 0), (known, i, st[i], ol[i], w)
            else:
                assert (st[i], ol[i]) == ("OK", len(w)), (known, i, st[i], ol[i])
                assert out[descs[i][1]: descs[i][1] + ol[i]].tobytes() == w, (known, i)


# ---------------------------------------------------------------- 5. where it writes
@pytest.mark.parametrize("nstates", [2, 1])
def test_regions_and_gaps(torch_cuda, shared, nstates):
    """Regions of exactly the payload, one byte less (never stored past), a
    few bytes more, and 16 bytes in all, 16 or 48 bytes apart; then the same
    for the decoder, with and without lengths."""
    torch = torch_cuda
    name = "trained-12"
    msgs = [m for m in messages(name, nstates, 63) if len(m) < 65535] + [data(name, n, 7) for n in (2, 100)]
    want = [ref(name, m, nstates) for m in msgs]
    caps = [max(len(w[0]) + (0, -1, 5, 16 - len(w[0]))[i % 4], 0) for i, w in enumerate(want)]
    descs, in_size, out_size = layout([len(m) for m in msgs], caps, gap=16)
    descs = [(so, oo + 32 * (i // 7), n, cap) for i, (so, oo, n, cap) in enumerate(descs)]
    st, cl, pb, out = device_call(torch, "compress", shared[name], nstates, descs, pack(descs, msgs, in_size),
                                  out_size + 32 * 10)
    assert_gaps(out, descs, "compress")
    for i, (w, cap) in enumerate(zip(want, caps)):
        if len(w[0]) > cap:
            assert (st[i], cl[i]) == ("DST_TOO_SMALL", 0), (i, st[i], cl[i], len(w[0]), cap)
        else:
            assert (st[i], cl[i], pb[i]) == ("OK", len(w[0]), w[1]), (i, st[i], cl[i], len(w[0]), cap)
            assert out[descs[i][1]: descs[i][1] + cl[i]].tobytes() == w[0], i
    assert {"OK", "DST_TOO_SMALL"} == set(st)
    pay = [w[0] for w in want]
    for known in (True, False):
        caps = [max(len(m) + (0, -1, 5)[i % 3], 0) for i, m in enumerate(msgs)]
        descs, in_size, out_size = layout([len(p) for p in pay], caps, gap=16)
        st, ol, _, out = device_call(torch, "decompress", shared[name], nstates, descs, pack(descs, pay, in_size),
                                     out_size, [len(m) for m in msgs] if known else None)
        assert_gaps(out, descs, "decompress")
        for i, (m, cap) in enumerate(zip(msgs, caps)):
            if len(m) > cap:
                assert (st[i], ol[i]) == ("DST_TOO_SMALL", 0), (known, i, st[i], ol[i])
            else:
                assert (st[i], ol[i]) == ("OK", len(m)), (known, i, st[i], ol[i])
                assert out[descs[i][1]: descs[i][1] + ol[i]].tobytes() == m, (known, i)


@pytest.mark.parametrize("nstates", [2, 1])
def test_random_payloads_stay_inside(torch_cuda, shared, nstates):
    """64 payloads of random bytes: a status or bytes, every gap intact."""
    torch = torch_cuda
    rng = np.random.default_rng(0xBAD5EED + nstates)
    pay = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 400, 64)]
    caps = [int(c) for c in rng.integers(0, 700, 64)]
    norm, L, tl = tables()["trained-11"]
    for known in (False, True):
        raw = [int(r) for r in rng.integers(0, 700, 64)] if known else None
        descs, in_size, out_size = layout([len(p) for p in pay], caps, gap=16)
        st, ol, _, out = device_call(torch, "decompress", shared["trained-11"], nstates, descs, pack(descs, pay, in_size),
                                     out_size, raw)
        assert_gaps(out, descs, "decompress of random bytes")
        for i, p in enumerate(pay):
            try:
                w = R.decompress_shared(p, norm, L, tl, nstates, raw_len=raw[i] if known else None, out_cap=caps[i])
            except SpecError as e:
                w = e.code
            if isinstance(w, str):
                assert (st[i], ol[i]) == (w, 0), (known, i, st[i], ol[i], w)
            else:
                assert (st[i], ol[i]) == ("OK", len(w)) and ol[i] <= caps[i], (known, i, st[i], ol[i], len(w))
                assert out[descs[i][1]: descs[i][1] + ol[i]].tobytes() == w, (known, i)
        assert len(set(st)) > 1


# ---------------------------------------------------------------- 6. stream order
def test_build_compress_decompress_behind_a_gate(torch_cuda):
    """One chain of build -> compress -> decompress on a non-blocking side
    stream, queued while its inputs do not exist yet (the pattern of
    tests/test_gpu_stream_order.py: poison first, the real inputs copied in
    behind the gate, no host synchronisation in the chain)."""
    from test_gpu_stream_order import GATE_CAP_MS, GATE_FACTOR, GATE_FLOOR_MS, Chain, Ctx, pinned, stream_ptr

    torch = torch_cuda
    name, nstates = "trained-11", 2
    lib = _lib.load()

    class SharedChain(Chain):
        def __init__(self):
            self.msgs = [data(name, n, 300 + n) for n in (2, 17, 300, 1000, 4099, 64)]
            self.want = [ref(name, m, nstates) for m in self.msgs]
            L = tables()[name][1]
            caps = [int(lib.fsehip_shared_out_bytes(len(m), L)) for m in self.msgs]
            self.enc, in_size, self.comp_size = layout([len(m) for m in self.msgs], caps)
            self.host_src = pack(self.enc, self.msgs, in_size)
            # the decoder reads the encoder's regions: lengths from the reference, known before the run
            self.dec, so = [], 0
            for (_, oo, n, _), (p, _) in zip(self.enc, self.want):
                self.dec.append((oo, so, len(p), n))
                so += (n + 15) // 16 * 16 + 64
            self.out_size = so

        def alloc(self, torch):
            self.torch = torch
            n = len(self.msgs)
            as_bytes = lambda descs: np.frombuffer(bytes((_lib.StreamDesc * n)(*[_lib.StreamDesc(*d) for d in descs])),  # noqa: E731
                                                   dtype=np.uint8)
            hosts = [np.frombuffer(bytes(nh_of(*tables()[name])), dtype=np.uint8), self.host_src, as_bytes(self.enc),
                     as_bytes(self.dec), np.array([len(m) for m in self.msgs], dtype=np.int32)]
            self.inputs = [torch.empty(len(h), dtype=torch.uint8 if h.dtype == np.uint8 else torch.int32, device="cuda")
                           for h in hosts]
            self.uploads = [(d, pinned(torch, h)) for d, h in zip(self.inputs, hosts)]
            self.nh, self.src, self.d_enc, self.d_dec, self.raw = self.inputs
            self.w_img, self.image = g8(torch, int(lib.fsehip_shared_table_bytes()))
            self.w_bst, self.bst = g32(torch, 1)
            self.w_comp, self.comp = g8(torch, self.comp_size)
            self.w_out, self.out = g8(torch, self.out_size)
            self.w32 = {k: g32(torch, n) for k in ("comp_len", "bits", "status", "out_len", "dec status")}

        def poison(self):
            self.src.fill_(7)
            for t in (self.nh, self.d_enc, self.d_dec, self.raw, self.image):  # an all-zero image is invalid
                t.zero_()
            self.comp.zero_()  # the decoder's input
            self.out.fill_(A5)
            self.bst.fill_(F32)
            for _, v in self.w32.values():
                v.fill_(F32)

        def enqueue(self, step9):
            hs, n, v = stream_ptr(self.torch), len(self.msgs), {k: x[1] for k, x in self.w32.items()}
            assert lib.fsehip_shared_table_build(ptr(self.nh), ptr(self.image), ptr(self.bst), hs) == 0
            assert lib.fsehip_compress_shared(nstates, ptr(self.image), ptr(self.src), ptr(self.d_enc), n, ptr(self.comp),
                                              ptr(v["comp_len"]), ptr(v["bits"]), ptr(v["status"]), hs) == 0
            assert lib.fsehip_decompress_shared(nstates, ptr(self.image), ptr(self.comp), ptr(self.d_dec), n,
                                                ptr(self.out), ptr(self.raw), ptr(v["out_len"]), ptr(v["dec status"]),
                                                hs) == 0
            step9()

        def check(self):
            for w, view, fill, what in ((self.w_img, self.image, A5, "image"), (self.w_bst, self.bst, F32, "build status"),
                                        (self.w_comp, self.comp, A5, "d_out"), (self.w_out, self.out, A5, "decode d_out")):
                assert_guards(w, view, fill, what)
            for k, (w, view) in self.w32.items():
                assert_guards(w, view, F32, k)
            v = {k: x[1].tolist() for k, x in self.w32.items()}
            assert self.bst.tolist() == [0] and v["status"] == [0] * len(self.msgs) == v["dec status"], v
            assert v["comp_len"] == [len(p) for p, _ in self.want] and v["bits"] == [b for _, b in self.want]
            assert v["out_len"] == [len(m) for m in self.msgs]
            comp, out = self.comp.cpu().numpy(), self.out.cpu().numpy()
            for (_, oo, _, _), (p, _), (_, do, _, n), m in zip(self.enc, self.want, self.dec, self.msgs):
                assert comp[oo: oo + len(p)].tobytes() == p and out[do: do + n].tobytes() == m

    ctx, chain = Ctx(torch), SharedChain()
    chain.alloc(torch)
    ctx.run(chain, gated=False)  # the first call of a kernel loads its code
    ms = ctx.run(chain, gated=False)
    ctx.gate_ms = min(GATE_CAP_MS, max(GATE_FACTOR * ms, GATE_FLOOR_MS))
    ctx.run(chain, gated=True)
