"""Shared-table coding without a GPU: the reference (tests/shared_ref.py)
pinned to the C oracle, NormHistogram's TryFrom, the before-the-device
argument checks of the fsehip_*_shared calls, and the new kernels' resources."""
import ctypes as C

import numpy as np
import pytest

import shared_ref as R
from entropy_coders_amd import _lib
from oracle import oracle as O
from oracle.spec import SpecError
from test_kernel_resources import kernel_metadata, workgroups_per_cu

LENGTHS = [2, 3, 4, 5, 17, 64, 255, 1024, 4097]
ALPHA = np.array([3, 9, 27, 81, 128, 200, 255], dtype=np.uint8)


def message(n, seed):
    """The bench's skewed generator from 64 bytes on, 7 symbols below."""
    if n >= 64:
        return O.generate(0, 0.155, 0x5EED0A00, seed, n).tobytes()
    m = ALPHA[np.random.default_rng(seed).integers(0, 7, n)]
    m[:2] = ALPHA[:2]  # two symbols at least
    return m.tobytes()


def own_table(m, L):
    nh, _ = O.normalize(O.hist_count(m), L)
    return list(nh.norm), int(nh.log2), int(nh.table_len)


# ---------------------------------------------------------------- the pin to the C oracle
@pytest.mark.parametrize("nstates", [2, 1])
@pytest.mark.parametrize("L", [9, 11, 12])
def test_own_table_payload_is_the_oracles_stream_minus_its_header(L, nstates):
    for i, n in enumerate(LENGTHS):
        m = message(n, 100 * L + i)
        stream, bits = O.compress2(m, L) if nstates == 2 else O.compress(m, L)
        _, used = O.header_read(stream)
        norm, log2, tl = own_table(m, L)
        payload, pbits = R.compress_shared(m, norm, log2, tl, nstates)
        assert payload == stream[used:], (n, L, nstates)
        assert pbits == bits, (n, L, nstates, pbits, bits)
        if n <= 1024:  # the bit-list reader is slow
            assert R.decompress_shared(payload, norm, log2, tl, nstates) == m
            assert R.decompress_shared(payload, norm, log2, tl, nstates, raw_len=n) == m
            # (a symbol above half the table has states that cost no bit, and a payload cut by one such
            # symbol is a valid shorter one: the skewed generator's largest share is 0.155)
            for wrong in (n - 1, n + 1) if n >= 64 else ():
                with pytest.raises(SpecError, match="LENGTH_MISMATCH"):
                    R.decompress_shared(payload, norm, log2, tl, nstates, raw_len=wrong)


def test_reference_statuses():
    m = message(300, 1)
    norm, L, tl = own_table(m, 11)
    absent = next(s for s in range(tl) if norm[s] == 0)
    for src, ns, want in ((b"", 2, "EMPTY"), (b"", 1, "EMPTY"), (m[:1], 2, "TOO_SHORT"), (bytes(65537), 2, "UNSUPPORTED"),
                          (m[:10] + bytes([absent]) + m[:5], 2, "SYMBOL_NOT_IN_TABLE"),
                          (m[:10] + bytes([tl]), 1, "SYMBOL_NOT_IN_TABLE")):
        with pytest.raises(SpecError, match=want):
            R.compress_shared(src, norm, L, tl, ns)
    one, bits = R.compress_shared(m[:1], norm, L, tl, 1)  # one byte at one state: the seed, finish, the marker
    assert bits == L + 1 and R.decompress_shared(one, norm, L, tl, 1) == m[:1]
    payload, _ = R.compress_shared(m, norm, L, tl, 2)
    for data, kw, want in ((b"", {}, "EMPTY"), (payload[:-1] + b"\0", {}, "NO_MARKER"), (b"\x01", {}, "TOO_SHORT"),
                           (payload, {"out_cap": 299}, "DST_TOO_SMALL"), (payload, {"raw_len": 1}, "LENGTH_MISMATCH"),
                           (payload, {"raw_len": 300, "out_cap": 299}, "DST_TOO_SMALL")):
        with pytest.raises(SpecError, match=want):
            R.decompress_shared(data, norm, L, tl, 2, **kw)
    single = [0] * 256
    single[65] = 1 << 9
    for ns in (1, 2):
        p, _ = R.compress_shared(b"A" * 37, single, 9, 66, ns)
        assert R.decompress_shared(p, single, 9, 66, ns, raw_len=37) == b"A" * 37
        with pytest.raises(SpecError, match="SINGLE_SYMBOL"):
            R.decompress_shared(p, single, 9, 66, ns)
    assert R.build_status(norm, L, tl) == "OK"
    assert R.build_status(norm, 13, tl) == "UNSUPPORTED" and R.build_status(norm, 16, tl) == "TABLELOG_RANGE"
    assert R.build_status(norm[:5] + [norm[5] + 1] + norm[6:], L, tl) == "BAD_TABLE"


def test_trained_table_codes_every_byte():
    norm, L, tl = R.train([message(4096, 7)], 11, 1)
    assert (L, tl) == (11, 256) and all(v != 0 for v in norm) and R.build_status(norm, L, tl) == "OK"
    m = bytes(range(256)) + message(100, 8)
    for ns in (1, 2):
        p, _ = R.compress_shared(m, norm, L, tl, ns)
        assert R.decompress_shared(p, norm, L, tl, ns, raw_len=len(m)) == m


# ---------------------------------------------------------------- NormHistogram: TryFrom<[i32; 256]>
def table(**entries):
    t = [0] * 256
    for k, v in entries.items():
        t[int(k[1:])] = v
    return t


TRY_FROM = [
    ("a-valid-table", table(s0=16, s1=8, s2=4, s3=4)),
    ("one-symbol", table(s0=32)),
    ("trailing-zeros-give-table_len", table(s3=1024, s200=1024)),
    ("last-index", table(s0=1, s255=1)),
    ("negative-entries-count-by-absolute-value", table(s0=29, s1=-1, s2=-1, s9=-1)),
    ("below-minus-one-too", table(s0=28, s5=-4)),
    ("a-log-outside-5..15-is-accepted-here", table(s0=2, s1=2)),
    ("a-log-of-20", table(s0=1 << 19, s1=1 << 19)),
    ("sum-not-a-power-of-two", table(s0=16, s1=8, s2=4, s3=3)),
    ("negative-sum-not-a-power-of-two", table(s0=16, s1=-1)),
    ("all-zero", table()),
]


@pytest.mark.parametrize("name,t", [pytest.param(n, t, id=n) for n, t in TRY_FROM])
def test_norm_histogram_try_from(name, t):
    lib = _lib.load()
    nh = _lib.NormHistogram()
    rc = lib.norm_histogram_try_from((C.c_int32 * 256)(*t), C.byref(nh))
    try:
        norm, L, tl = R.try_from(t)
    except SpecError as e:
        assert _lib.STATUS[rc] == e.code == "BAD_TABLE"
        return
    assert rc == 0 and (list(nh.norm), nh.log2, nh.table_len) == (norm, L, tl)
    assert 1 << L == sum(abs(x) for x in t) and tl == max(i for i in range(256) if t[i]) + 1


def test_norm_histogram_try_from_python_call():
    from entropy_coders_amd import FseError, norm_histogram_try_from

    nh = norm_histogram_try_from(table(s0=16, s7=-1, s8=15))
    assert (nh.log2, nh.table_len, nh.norm[7]) == (5, 9, -1)
    with pytest.raises(FseError) as e:
        norm_histogram_try_from(table(s0=3))
    assert e.value.code == "BAD_TABLE"


# ---------------------------------------------------------------- argument checks before any device use
OK = C.c_void_p(4096)
ODD = C.c_void_p(4096 + 8)
ROWS = []


def row(name, want, call):
    ROWS.append(pytest.param(call, want, id=name))


row("try_from-null-table", "BAD_ARG", lambda lib: lib.norm_histogram_try_from(None, C.byref(_lib.NormHistogram())))
row("try_from-null-out", "BAD_ARG", lambda lib: lib.norm_histogram_try_from((C.c_int32 * 256)(32), None))

# fsehip_shared_table_build(d_nh, d_table, d_status, stream)
row("table_build-null-nh", "BAD_ARG", lambda lib: lib.fsehip_shared_table_build(None, OK, OK, None))
row("table_build-null-table", "BAD_ARG", lambda lib: lib.fsehip_shared_table_build(OK, None, OK, None))
row("table_build-null-status", "BAD_ARG", lambda lib: lib.fsehip_shared_table_build(OK, OK, None, None))
row("table_build-table-misaligned", "BAD_ARG", lambda lib: lib.fsehip_shared_table_build(OK, ODD, OK, None))


# fsehip_compress_shared(nstates, d_table, d_src, d_desc, n_msgs, d_out, d_comp_len, d_payload_bits, d_status, stream)
def cs(nstates=2, tab=OK, src=OK, desc=OK, n=4, out=OK, clen=OK, status=OK):
    return lambda lib: lib.fsehip_compress_shared(nstates, tab, src, desc, n, out, clen, None, status, None)


# fsehip_decompress_shared(nstates, d_table, d_in, d_desc, n_msgs, d_out, d_raw_len, d_out_len, d_status, stream)
def ds(nstates=2, tab=OK, src=OK, desc=OK, n=4, out=OK, clen=OK, status=OK):
    return lambda lib: lib.fsehip_decompress_shared(nstates, tab, src, desc, n, out, None, clen, status, None)


for name, f in (("compress_shared", cs), ("decompress_shared", ds)):
    row(f"{name}-no-messages", "OK", f(n=0))
    row(f"{name}-no-messages-before-nstates", "OK", f(n=0, nstates=3))
    row(f"{name}-no-messages-before-null", "OK", f(n=0, tab=None))
    row(f"{name}-nstates-3", "BAD_ARG", f(nstates=3))
    for arg in ("tab", "src", "desc", "out", "clen", "status"):
        row(f"{name}-null-{arg}", "BAD_ARG", f(**{arg: None}))
    for arg in ("tab", "src", "out"):
        row(f"{name}-{arg}-misaligned", "BAD_ARG", f(**{arg: ODD}))
    row(f"{name}-too-many", "UNSUPPORTED", f(n=(1 << 24) + 1))
    row(f"{name}-2^24-is-not-too-many-but-null", "BAD_ARG", f(n=1 << 24, src=None))
    row(f"{name}-null-before-too-many", "BAD_ARG", f(n=(1 << 24) + 1, src=None))


@pytest.mark.parametrize("call,want", ROWS)
def test_malformed_call(call, want):
    assert _lib.STATUS[call(_lib.load())] == want


def test_layout_helpers():
    lib = _lib.load()
    assert lib.fsehip_shared_table_bytes() == 64 + 2048 + 8192 + 16384  # the small parts, tt, stateTable, decode table
    for n, L in ((0, 11), (1, 5), (512, 11), (65536, 12)):
        assert lib.fsehip_shared_out_bytes(n, L) == ((n * L + 2 * L + 1 + 7) // 8 + 15) // 16 * 16
    assert lib.fsehip_shared_out_bytes(100, 0) == lib.fsehip_shared_out_bytes(100, 5)
    assert lib.fsehip_shared_out_bytes(100, 15) == lib.fsehip_shared_out_bytes(100, 12)
    assert _lib.STATUS[-20] == "SYMBOL_NOT_IN_TABLE"


# ---------------------------------------------------------------- the kernels' resources
# (kernel, LDS bytes, workgroups per CU): the tables once per 256-thread
# workgroup, so 8 workgroups (the CU's 32 waves) stay resident -- 2,048 chains
# per CU -- and the one-wave build keeps 15.
GUARDS = [
    ("_ZN6fsehip20shared_encode_kernelILi2EE", 10272, 8),
    ("_ZN6fsehip20shared_encode_kernelILi1EE", 10272, 8),
    ("_ZN6fsehip20shared_decode_kernelILi2EE", 16384, 8),
    ("_ZN6fsehip20shared_decode_kernelILi1EE", 16384, 8),
    ("_ZN6fsehip19shared_build_kernelE", 10752, 15),
]


@pytest.fixture(scope="module")
def meta():
    return kernel_metadata(_lib.LIB_PATH)


@pytest.mark.parametrize("prefix,lds,wgs", GUARDS)
def test_shared_kernel_resources(meta, prefix, lds, wgs):
    hits = [k for k in meta if k.startswith(prefix)]
    assert len(hits) == 1, (prefix, hits)
    md = meta[hits[0]]
    assert md.get(".private_segment_fixed_size", 0) == 0, "register spills to scratch"
    assert md[".group_segment_fixed_size"] == lds, (prefix, md[".group_segment_fixed_size"])
    waves = -(-md[".max_flat_workgroup_size"] // 64)
    resident = min(workgroups_per_cu(md), 32 // waves)  # LDS and registers, and the CU's 32 waves
    assert resident == wgs, (prefix, md[".group_segment_fixed_size"], md[".vgpr_count"])
