"""The caller-built histograms and tables of tests/caller_cases.py on the
CPU: every case takes the exit it was built for, and the two restatements of
the crate (oracle/fse_oracle.c, oracle/spec.py) agree on every value the GPU
tests (tests/test_gpu_caller_tables.py) then hold the device to."""
import collections

import numpy as np
import pytest

import caller_cases as CC
import shared_ref as R
from oracle import oracle as O
from oracle import spec

# Every exit the constructions and the search reach; a later edit that loses
# one fails test_labels_reached.
REQUIRED = [
    "single", "fast+", "fast-", "fast0",
    "slow:prop",        # at most 65,536 counts, and at 1,431,655,765 (the last size whose size * 3 fits)
    "slow:r2,prop",     # at most 65,536 counts, and at 1,431,655,765 / 766, 2^31, 2^32 - 1
    "slow:r2,cursed",   # 2^31 and 2^32 - 1: FSE_ERR_CURSED from a consistent histogram
]
# Not reached, with a consistent histogram (counts sum to size, table_len right
# behind the last count).  L >= ilog2(table_len - 1) + 2 gives table_len <=
# 2^(L-1) =: H, and a wrapped product is never above the true one, so the wraps
# only lower low_one and low:
#   slow:td0        the first pass marks at most table_len <= H symbols, one
#                   slot each, so to_distribute >= 2^L - H = H > 0.
#   slow:allmarked, slow:total0(cursed)
#                   both need every count marked.  Marked in the first pass
#                   means t <= low_one <= 1.5 * size / 2^L, at most H of them:
#                   <= 0.75 * size in all, so some mass stays.  The second
#                   round marks u symbols of t <= low <= 1.5 * total / td each;
#                   marking all of them needs u >= td / 1.5, but u <= H - m and
#                   td = 2^L - m (m marked before) give 1.5 * (H - m) >= 2H - m,
#                   i.e. -0.5 * H >= 0.5 * m: never.
#   slow:cursed     (no second round) not met: 30,000 random histograms of at
#                   most 65,536 counts and 300 per family at the large sizes
#                   gave none; no argument that it cannot happen, so it is not
#                   required and a case that reaches it would be welcome.
#   slow:prop at size >= 1,431,655,766
#                   the wrapped low_one is below half a slot there (size * 3 -
#                   2^32 < size up to 2^32 * 2 / 3, size * 3 - 2^33 < size
#                   above), and the unmarked mass per free slot starts at one
#                   slot and only grows when a -1 symbol (at most one slot of
#                   mass) leaves: total / to_distribute > low_one always, the
#                   second round always runs.  The plain exit is held right
#                   below the wrap instead (below_wrap_prop_*), and the same
#                   seed one count later is slow:r2,prop (at_wrap_r2_prop_*).
# A histogram whose size disagrees with its counts can reach some of these;
# none is included: 20,000 random ones with size 0.3 .. 2 times the counts
# reached no new exit.


def _hist(counts, size, table_len):
    h = O.Hist()
    for i, c in enumerate(counts):
        h.counts[i] = c
    h.size, h.table_len = size, table_len
    return h


def oracle_normalize(counts, size, table_len, log2):
    """(norm list, log, table_len, used_slow) or a status name."""
    try:
        nh, slow = O.normalize(_hist(counts, size, table_len), log2)
    except O.OracleError as e:
        return e.code
    return list(nh.norm), nh.log2, nh.table_len, slow


def spec_normalize(counts, size, table_len, log2):
    try:
        norm, L, slow = spec.normalize(counts, size, table_len, log2)
    except spec.SpecError as e:
        return e.code
    return norm, L, table_len, slow


def norm_struct(table, L, table_len):
    nh = O.Norm()
    for i, v in enumerate(table):
        nh.norm[i] = v
    nh.log2, nh.table_len = L, table_len
    return nh


@pytest.mark.parametrize("case", CC.HIST_CASES, ids=[c[0] for c in CC.HIST_CASES])
def test_histogram_case(case):
    name, counts, size, tl, log2, label = case
    assert CC.normalize_exit(counts, size, tl, log2) == label
    assert CC.consistent(case), "a case outside the crate's own domain must be marked as such"
    a, b = oracle_normalize(counts, size, tl, log2), spec_normalize(counts, size, tl, log2)
    assert a == b, name
    if label.endswith("cursed"):
        assert a == "CURSED"
    else:
        norm, L, _, slow = a
        assert L == CC.effective_log(tl, log2) and slow == label.startswith("slow")
        assert sum(abs(v) for v in norm) == 1 << L and all(v == 0 for v in norm[tl:])


def test_labels_reached():
    reached = collections.Counter(c[5] for c in CC.HIST_CASES)
    print("labels reached:", dict(reached))
    assert set(reached) >= set(REQUIRED), set(REQUIRED) - set(reached)
    small = {c[5] for c in CC.HIST_CASES if c[2] <= 65536}
    assert small >= {"single", "fast+", "fast-", "fast0", "slow:prop", "slow:r2,prop"}
    wrapped = {c[5] for c in CC.HIST_CASES if c[2] >= CC.WRAP3}
    assert wrapped >= {"slow:r2,prop", "slow:r2,cursed"}
    assert {c[2] for c in CC.HIST_CASES} >= {CC.WRAP3 - 1, CC.WRAP3, 1 << 31, (1 << 32) - 1}
    below = {c[5] for c in CC.HIST_CASES if c[2] == CC.WRAP3 - 1}
    assert "slow:prop" in below
    # the clamp and the raise: table_len 2, 3, 129, 255, 256 at requested logs 0, 5, 15, 20
    seen = {(c[3], c[4]) for c in CC.HIST_CASES}
    assert seen >= {(tl, lg) for tl in (2, 3, 129, 255, 256) for lg in (0, 5, 15, 20)}


def test_wrap_matters():
    """In every case from the wrap on, low_one with the wrap differs from
    low_one without it, so normalize_slow there runs on the wrapped value."""
    changed = 0
    for name, counts, size, tl, log2, label in CC.HIST_CASES:
        if size < CC.WRAP3:
            continue
        L = CC.effective_log(tl, log2)
        assert ((size * 3) & CC.M32) >> (L + 1) != (size * 3) >> (L + 1), name
        changed += 1
    assert changed >= 8


def test_rounding_table_case():
    for name in ("rtb_straddle", "rtb_straddle_2_32m1"):
        case = next(c for c in CC.HIST_CASES if c[0] == name)
        norm = oracle_normalize(*case[1:5])[0]
        assert len(CC.RTB_WANT[name]) == 14
        for s, v in CC.RTB_WANT[name].items():
            assert norm[s] == v, (name, s, case[1][s], v, norm[s])
    p0 = next(c for c in CC.HIST_CASES if c[0] == "rtb_p0_above_2_31")
    assert oracle_normalize(*p0[1:5])[0][9] == 1  # floor 0, any remainder beats 0


def test_tie_goes_to_the_first_symbol():
    for name, first, others in (("tie_three_lanes", 1, (9, 20)), ("tie_last_lane", 130, (255,)),
                                ("tie_negative_residue", 64, (200,))):
        case = next(c for c in CC.HIST_CASES if c[0] == name)
        assert case[1][first] == max(case[1]) and all(case[1][o] == case[1][first] for o in others)
        assert first // 4 not in {o // 4 for o in others}  # different lanes
        norm = oracle_normalize(*case[1:5])[0]
        assert all(norm[o] != norm[first] for o in others), name
        resid = norm[first] - norm[others[0]]
        assert resid != 0 and (resid > 0) == (case[5] == "fast+")


def test_slow_boundary():
    exact = next(c for c in CC.HIST_CASES if c[0] == "slow_boundary_exact")
    minus = next(c for c in CC.HIST_CASES if c[0] == "slow_boundary_minus_one")
    assert oracle_normalize(*exact[1:5])[3] is True and oracle_normalize(*minus[1:5])[3] is False
    # the fast pass of `exact`: two symbols of 15 and nine of -1 at log 5: -to_distribute = 7 = 15 >> 1
    assert 32 - (15 + 15 + 9) == -(15 >> 1) and 32 - (15 + 15 + 8) == -(15 >> 1) + 1


@pytest.mark.parametrize("case", CC.OPTIMAL_CASES, ids=[c[0] for c in CC.OPTIMAL_CASES])
def test_optimal_case(case):
    name, counts, size, tl = case
    assert sum(counts) == size
    L = O.optimal_log2(_hist(counts, size, tl))
    assert L == spec.optimal_log2(size, tl)
    if size <= 4:  # max_bits wraps to a huge u32: min(11, ..) = 11
        assert L == 11
    assert oracle_normalize(counts, size, tl, L) == spec_normalize(counts, size, tl, L)


def test_optimal_sizes():
    assert {c[2] for c in CC.OPTIMAL_CASES} >= {2, 3, 4, 5, (1 << 32) - 1}


TABLES = CC.TABLE_CASES + [(n, t) for n, t, _ in CC.STRUCT_CASES]
TABLE_LENS = {n: tl for n, _, tl in CC.STRUCT_CASES}


@pytest.mark.parametrize("case", TABLES, ids=[c[0] for c in TABLES])
def test_table_case(case):
    name, table = case
    assert len(table) == 256 and all(v >= -1 for v in table)
    norm, L, tl = R.try_from(table)
    assert 5 <= L <= 15
    tl = TABLE_LENS.get(name, tl)
    nh = norm_struct(table, L, tl)
    head = O.header_write(nh)
    assert head == spec.header_write(norm, L, tl)
    if name in TABLE_LENS:  # the `remaining <= 1` break: nothing is written for the entries behind the last count
        assert head == spec.header_write(norm, L, R.try_from(table)[2])
    for tail in (b"", bytes(range(7))):
        back, used = O.header_read(head + tail)
        assert list(back.norm) == norm and back.log2 == L and used == len(head)
        assert back.table_len == R.try_from(table)[2]
        assert spec.header_read(head + tail) == (norm, L, back.table_len, len(head))
    log2, st, dnb, dfs, spread = O.ctable(nh)
    s_st, s_dnb, s_dfs = spec.encode_table(norm, L, tl)
    assert log2 == L and list(st) == s_st and list(spread) == spec.spread(norm, L, tl)
    assert [int(x) for x in dnb] == s_dnb and [int(x) for x in dfs] == s_dfs
    log2, ns, sym, nb = O.dtable_nh(nh)
    s_dt = spec.decode_table(norm, L, tl)
    assert log2 == L and [(int(a), int(b), int(c)) for a, b, c in zip(ns, sym, nb)] == s_dt


def test_table_shapes():
    """The shapes the issue names are all there."""
    by = dict(CC.TABLE_CASES)
    logs = {n: R.try_from(t)[1] for n, t in CC.TABLE_CASES}
    assert all(v in (0, -1) for v in by["all_low_32_L5"]) and logs["all_low_32_L5"] == 5
    for n in ("all_low_32_L5", "all_low_256_L8", "ones_256_L8"):  # log below ilog2(table_len - 1) + 2
        tl = R.try_from(by[n])[2]
        assert logs[n] < (tl - 1).bit_length() - 1 + 2
    for n, t in CC.TABLE_CASES:
        L = logs[n]
        if n.startswith("half_minus_one"):
            assert max(t) == (1 << (L - 1)) - 1
        elif n.startswith("half"):
            assert max(t) == 1 << (L - 1)
    assert sorted(by["big_and_low_L5"][:2]) == [-1, 31] and (1 << 15) - 1 in by["low_and_big_L15"]
    runs = set()
    for n, t in CC.TABLE_CASES:
        nz = CC.table_alphabet(t)
        runs |= {b - a - 1 for a, b in zip(nz, nz[1:])}
    assert runs >= {1, 2, 3, 4, 23, 24, 25, 27, 48, 51, 253}
    longest = by["longest_header_L15"]
    n = len(O.header_write(norm_struct(longest, 15, 256)))
    print("longest header:", n, "bytes")
    assert R.try_from(longest)[1:] == (15, 256) and 440 <= n <= ((256 * 15) >> 3) + 3  # write_bound (histogram.rs:331)


def test_truncated_headers_agree():
    """NormHistogram::read on every prefix the GPU test uses: the two
    restatements agree on status, consumed bytes and the parsed table.  A
    header needs all its bytes (its last field ends in the last one), so every
    shorter prefix is an error on both; what the fallback of histogram.rs:
    471-473 decides is the header with no byte behind it when its last field
    is the 1-bit form of a final -1 and ends on a byte boundary: the
    fallback_* tables, which a reader without the fallback refuses."""
    for name, table in CC.TABLE_CASES:
        norm, L, tl = R.try_from(table)
        head = spec.header_write(norm, L, tl)
        for k in CC.prefix_lengths(len(head)):
            try:
                nh, used = O.header_read(head[:k])
                a = (list(nh.norm), nh.log2, nh.table_len, used)
            except O.OracleError as e:
                a = e.code
            try:
                b = spec.header_read(head[:k])
            except spec.SpecError as e:
                b = e.code
            assert a == b, (name, k)
            assert isinstance(a, str) == (k < len(head)), (name, k, a)
            if name.startswith("fallback"):
                assert table[tl - 1] == -1


def test_stream_construction():
    """A header plus compress_shared's payload is the crate's stream: with a
    block's own normalised histogram it equals the oracle's compress2 /
    compress, and the oracle decodes it."""
    src = O.generate(0, 0.155, 0xCA11, 0, 4097)
    nh = O.norm_new(src)
    norm, L, tl = list(nh.norm), nh.log2, nh.table_len
    for nstates, comp, dec in ((2, O.compress2, O.decompress2), (1, O.compress, O.decompress)):
        stream = spec.header_write(norm, L, tl) + R.compress_shared(src.tobytes(), norm, L, tl, nstates)[0]
        assert stream == comp(src)[0]
        assert dec(stream, CC.STREAM_CAP) == src.tobytes()


def test_table_streams():
    recs = CC.table_streams()
    made = [r for r in recs if r["stream"] is not None]
    print("streams:", len(made), "of", len(recs), "; not written:",
          sorted({(r["name"], r["status"]) for r in recs if r["stream"] is None}))
    print("oracle decode statuses:", dict(collections.Counter(r["want"] for r in made if isinstance(r["want"], str))))
    assert len(made) >= len(recs) * 3 // 4
    exact = [r for r in made if r["want"] == r["message"]]
    assert len(exact) >= len(made) // 2
    for r in made:  # the spec's decoder agrees with the oracle's wherever it ends within the bound
        if not isinstance(r["want"], str):
            got = (spec.decompress2 if r["nstates"] == 2 else spec.decompress)(r["stream"])
            assert got == r["want"], (r["name"], r["nstates"], r["n"])
