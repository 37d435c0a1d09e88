"""Histograms and normalised tables that a caller can hand to the building
blocks (include/fsehip.h section 1b) but that no sampled block produces, and
a labelled restatement of Histogram::normalize / normalize_slow
(histogram.rs:95-261) that says which exit a histogram takes.

The labeller produces no value under test: expected counts, headers and
tables come from oracle/oracle.py and oracle/spec.py.  It only names the
branch a case exercises, so that tests/test_caller_cases.py can hold the set
of branches reached and a later edit cannot lose one silently.

Everything here is plain Python and runs at import in well under a second:
cases are built by construction, or by a seeded search whose first seed is the
one that hits (the search only re-finds a case should the generator change).
"""
from __future__ import annotations

import random

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
RTB = [0, 473195, 504333, 520860, 550000, 700000, 750000, 830000]  # histogram.rs:100
LOG_MIN, LOG_MAX = 5, 15
WRAP3 = 1431655766  # the least size with size * 3 >= 2^32


def _ilog2(x: int) -> int:
    assert x > 0
    return x.bit_length() - 1


def _i32(x: int) -> int:
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def effective_log(table_len: int, log2: int) -> int:
    """histogram.rs:96-98: the clamp into 5..15, then the raise."""
    return max(min(max(log2, LOG_MIN), LOG_MAX), _ilog2(table_len - 1) + 2)


# ---------------------------------------------------------------- the labeller
def normalize_exit(counts, size, table_len, log2) -> str:
    """Which exit of histogram.rs:95-261 (release build: u32 / u64 / i32
    arithmetic wraps) this histogram takes at this requested log:

      single            t == size (113-120)
      fast+ fast- fast0 the fast path, by the sign of the residue (144-148)
      slow:td0          to_distribute == 0 after the first pass (183-189)
      slow:allmarked    every symbol marked (203-220)
      slow:total0       total == 0, the round-robin exit (221-235)
      slow:total0cursed the same with no positive entry to grow: the crate
                        loops forever there, both restatements report CURSED
      slow:prop         the proportional exit (236-253)
      slow:cursed       its panic (247-249)

    with `r2,` in front of the exit's name (slow:r2,prop) when the second
    marking round (192-201) ran."""
    assert table_len >= 2 and size >= 1  # ilog2(0) at 98 and the division at 103 panic
    L = effective_log(table_len, log2)
    scale = 62 - L
    step = (1 << 62) // size
    v_step = 1 << (scale - 20)
    low_t = size >> L
    td = 1 << L
    largest_p = 0
    for i in range(table_len):
        t = counts[i]
        if t == size:
            return "single"
        if t == 0:
            continue
        if t <= low_t:
            td = _i32(td - 1)
            continue
        prod = (t * step) & M64
        p = prod >> scale
        if p < 8:
            p += 1 if ((prod - (p << scale)) & M64) > v_step * RTB[p] else 0
        p = _i32(p)
        if p > largest_p:
            largest_p = p
        td = _i32(td - p)
    if not (td != 0 and _i32(-td) >= (largest_p >> 1)):
        return "fast+" if td > 0 else "fast-" if td < 0 else "fast0"

    low_one = ((size * 3) & M32) >> (L + 1)
    norm = [0] * 256
    UN = -2
    td = 1 << L
    total = size
    for s in range(table_len):
        t = counts[s]
        if t == 0:
            continue
        if t <= low_t:
            norm[s], td, total = -1, (td - 1) & M32, (total - t) & M32
        elif t <= low_one:
            norm[s], td, total = 1, (td - 1) & M32, (total - t) & M32
        else:
            norm[s] = UN
    if td == 0:
        return "slow:td0"
    r2 = ""
    if total // td > low_one:
        r2 = "r2,"
        low = ((total * 3) & M32) // ((td * 2) & M32)
        for s in range(table_len):
            if norm[s] == UN and counts[s] <= low:
                norm[s], td, total = 1, (td - 1) & M32, (total - counts[s]) & M32
    if ((1 << L) - td) & M32 == table_len:
        return f"slow:{r2}allmarked"
    if total == 0:
        return f"slow:{r2}total0" if any(v > 0 for v in norm[:table_len]) or td == 0 else f"slow:{r2}total0cursed"
    vsl = 62 - L
    mid = (1 << (vsl - 1)) - 1
    r_step = ((((1 << vsl) * td) & M64) + mid) // total
    acc = mid
    for s in range(table_len):
        if norm[s] == UN:
            end = (acc + ((counts[s] * r_step) & M64)) & M64
            if ((end >> vsl) - (acc >> vsl)) & M64 < 1:
                return f"slow:{r2}cursed"
            acc = end
    return f"slow:{r2}prop"


# ---------------------------------------------------------------- histogram cases
def _hist(pairs, size=None):
    """counts[256] from {symbol: count}; (counts, size, table_len)."""
    counts = [0] * 256
    for s, c in dict(pairs).items():
        counts[s] = c
    return counts, sum(counts) if size is None else size, max(s for s in range(256) if counts[s]) + 1


def _random_hist(rng: random.Random, size: int, table_len: int, nsym: int, sigma: float, ones: int = 0):
    """A consistent histogram of `size`: nsym symbols below table_len (the
    last one included) with log-normal weights, `ones` of them at count 1."""
    syms = sorted(rng.sample(range(table_len - 1), nsym - 1)) + [table_len - 1]
    rng.shuffle(syms)
    small, big = syms[:ones], syms[ones:]
    w = [2.718281828 ** rng.gauss(0.0, sigma) for _ in big]
    rest = size - len(small)
    counts = [0] * 256
    for s in small:
        counts[s] = 1
    for s, x in zip(big, w):
        counts[s] = max(1, int(x / sum(w) * rest))
    top = max(big, key=lambda s: counts[s])
    counts[top] += size - sum(counts)
    assert counts[top] >= 1 and sum(counts) == size
    return counts, size, table_len


def _search(label, size, log2, table_len, nsym, sigma, ones, seed, tries=4000):
    """The first seed from `seed` on whose histogram exits at `label`."""
    for k in range(tries):
        h = _random_hist(random.Random(seed + k), size, table_len, nsym, sigma, ones)
        if normalize_exit(*h, log2) == label:
            return h
    raise AssertionError(f"no {label} histogram at size {size} log {log2} from seed {seed}")


def _rtb_case(size):
    """At log 9, for p = 1..7 the largest count that still stays at p
    (remainder <= rest_to_beat) and the next one, which rounds up to p + 1;
    the filler symbol takes the residue, so every straddling count keeps its
    own value.  At size 65,536 step is 2^46 exactly and one slot is 128 counts,
    so a count is 8,192 units of the table's 2^-20; at 2^32 - 1 a count is an
    eighth of a unit, and an entry that is off by one unit moves the edge.
    p = 0 has no 'just under': its rest_to_beat is 0 and a count above
    low_threshold leaves a positive remainder, so it always becomes 1
    (_p0_case is its 'just over')."""
    L = 9
    scale, step = 62 - L, (1 << 62) // size
    v_step = 1 << (scale - 20)
    counts = [0] * 256
    s = 1
    want = {}
    for p in range(1, 8):
        under = ((p << scale) + v_step * RTB[p]) // step
        for t, v in ((under, p), (under + 1, p + 1)):
            assert (t * step) >> scale == p and ((t * step - (p << scale)) > v_step * RTB[p]) == (v == p + 1)
            counts[s], want[s] = t, v
            s += 3  # straddling counts in different lanes
    counts[0] = size - sum(counts)
    return (counts, size, s - 2), want


RTB_WANT: dict = {}


def _p0_case():
    """A count above low_threshold whose floor probability is 0: step's
    truncation has to outweigh the count's excess over one slot, which needs
    size > 2^31.  Found by walking sizes = 31 mod 32
    down from 2^32 - 1 at log 5."""
    L, scale = 5, 57
    for size in range((1 << 32) - 1, (1 << 32) - (1 << 16), -32):
        t = (size >> L) + 1
        if (t * ((1 << 62) // size)) >> scale == 0:
            return _hist({0: size - t, 9: t})
    raise AssertionError("no p = 0 count found")


def _build_hist_cases():
    cases = []

    def add(name, h, log2, label):
        cases.append((name, h[0], h[1], h[2], log2, label))

    # -- every exit a consistent histogram of at most 65,536 counts reaches
    add("single", _hist({7: 4096}), 11, "single")
    add("fast_plus", _hist({0: 3000, 1: 2000, 2: 1000, 40: 17}), 9, "fast+")
    add("fast_minus", _hist({1: 1000, 9: 1000, **{20 + k: 1 for k in range(8)}}), 5, "fast-")
    add("fast_zero", _hist({0: 2048, 1: 1024, 2: 512, 3: 512}), 5, "fast0")
    # 12 symbols of count 1 take 12 slots for no mass: the 4 heavy symbols
    # overshoot (slow), and the 20 slots left carry 1.6 slots of mass each
    # (> low_one = 1.5 slots), so the second round runs and marks nobody ...
    add("r2_prop_none_marked", _hist({**{k: 1 for k in range(12)}, 12: 1000, 13: 1000, 14: 1000, 15: 1000}), 5,
        "slow:r2,prop")
    # ... and here it marks symbol 12 (2 slots of mass <= low = 2.4 slots)
    add("r2_prop_one_marked", _hist({**{k: 1 for k in range(12)}, 12: 250, 13: 1250, 14: 1250, 15: 1250}), 5,
        "slow:r2,prop")
    add("slow_prop_search", _search("slow:prop", 65536, 9, 200, 150, 1.5, 0, 3), 9, "slow:prop")
    add("slow_prop_search_L5", _search("slow:prop", 4001, 5, 16, 14, 1.0, 3, 5), 5, "slow:prop")
    add("r2_prop_search_L9", _search("slow:r2,prop", 65536, 9, 256, 256, 2.0, 0, 3), 9, "slow:r2,prop")

    # -- the slow path's boundary: -to_distribute == largest_prob >> 1 exactly,
    # and one short of it.  Two symbols of 15 slots each, k symbols of count 1.
    add("slow_boundary_exact", _hist({1: 1000, 2: 1000, **{4 + k: 1 for k in range(9)}}), 5, "slow:prop")
    add("slow_boundary_minus_one", _hist({1: 1000, 2: 1000, **{4 + k: 1 for k in range(8)}}), 5, "fast-")

    # -- a tie on the largest probability across lanes (lane = symbol // 4):
    # symbols 1, 9 and 20 at 10 slots each, the residue of 2 goes to symbol 1
    add("tie_three_lanes", _hist({1: 1000, 9: 1000, 20: 1000}), 5, "fast+")
    add("tie_last_lane", _hist({3: 500, 130: 9000, 255: 9000, 7: 500}), 12, "fast+")
    add("tie_negative_residue", _hist({64: 1000, 200: 1000, **{k: 1 for k in range(8)}}), 8, "fast-")

    # -- the rounding table
    for size, name in ((65536, "rtb_straddle"), (M32, "rtb_straddle_2_32m1")):
        h, want = _rtb_case(size)
        RTB_WANT[name] = want
        add(name, h, 9, "fast+")
    add("rtb_p0_above_2_31", _p0_case(), 5, "fast+")

    # -- table_len 2, 3, 129, 255, 256 at requested logs 0, 5, 15, 20
    for tl in (2, 3, 129, 255, 256):
        rng = random.Random(0xC0DE + tl)
        h = _random_hist(rng, 65536 if tl > 3 else 1000 + tl, tl, min(tl, 2 + tl // 2), 1.0)
        for log2 in (0, 5, 15, 20):
            add(f"tl{tl}_log{log2}", h, log2, "fast+")

    # -- size * 3 and total * 3 wrap from WRAP3 on: both sides of it, 2^31 and
    # 2^32 - 1.  From WRAP3 on the wrapped low_one is below half a slot while
    # the unmarked mass per free slot never falls below one slot (a -1 symbol
    # frees at most its own slot's worth), so the second round always runs
    # there: a plain slow:prop exists only below the wrap, and the same seed
    # one count further is slow:r2,prop.
    fam = {"A": (5, 16, 14, 1.0, 3), "B": (9, 256, 200, 1.2, 100), "C": (9, 256, 256, 2.0, 0),
           "D": (5, 16, 16, 1.0, 10)}
    for size, tag in ((WRAP3 - 1, "below_wrap"), (WRAP3, "at_wrap"), (1 << 31, "2_31"), (M32, "2_32m1")):
        for label, f, seed in BIG[tag]:
            log2, tl, nsym, sigma, ones = fam[f]
            name = f"{tag}_{label.split(':')[1].replace(',', '_')}_{f}"
            add(name, _search(label, size, log2, tl, nsym, sigma, ones, seed, 200), log2, label)
    return cases


# (label, family, first seed that hits), from a census of 300 seeds per family and size
_WRAPPED = [("slow:r2,prop", "A", 5), ("slow:r2,cursed", "A", 76), ("slow:r2,cursed", "B", 1), ("slow:r2,prop", "B", 3),
            ("slow:r2,cursed", "C", 1), ("slow:r2,prop", "C", 23)]
BIG = {
    "below_wrap": [("slow:prop", "A", 5), ("slow:prop", "B", 1), ("slow:r2,prop", "D", 5), ("slow:r2,prop", "C", 3)],
    "at_wrap": [("slow:r2,prop", "A", 5), ("slow:r2,prop", "B", 1), ("slow:r2,prop", "C", 1)],
    "2_31": _WRAPPED,
    "2_32m1": _WRAPPED,
}

HIST_CASES = _build_hist_cases()

# normalize_optimal: (name, counts, size, table_len); sizes 2..4 wrap max_bits (histogram.rs:271)
OPTIMAL_CASES = [
    ("opt_size2", *_hist({0: 1, 1: 1})),
    ("opt_size3", *_hist({0: 2, 5: 1})),
    ("opt_size4", *_hist({2: 1, 3: 3})),
    ("opt_size4_wide", *_hist({0: 1, 100: 1, 200: 1, 255: 1})),
    ("opt_size5", *_hist({0: 2, 1: 2, 17: 1})),
    ("opt_2_32m1_two", *_hist({0: M32 - 12345, 1: 12345})),
    ("opt_2_32m1_wide", *_random_hist(random.Random(0x0F7), M32, 256, 256, 1.5)),
]


def consistent(case) -> bool:
    """Counts that sum to size and a table_len right behind the last count:
    what Histogram::new produces.  Every case above is; one that is not would
    be outside the crate's own domain and has to say so in its name."""
    _, counts, size, table_len, _, _ = case
    return sum(counts) == size and table_len == max(s for s in range(256) if counts[s]) + 1


# ---------------------------------------------------------------- table cases
def _table(pairs):
    t = [0] * 256
    for s, v in dict(pairs).items():
        t[s] = v
    return t


def _runs_table(runs, first, rest):
    """Present symbols separated by zero runs of the given lengths."""
    t = [0] * 256
    s = 0
    t[s] = first
    for r, v in zip(runs, rest):
        s += r + 1
        t[s] = v
    return t


def _longest_header():
    """Log 15, table_len 256.  A field has num_bits or num_bits - 1 bits and
    num_bits falls as `remaining` halves, so a long header keeps `remaining`
    above 2^14 (15-bit fields after the first) and its values at or above
    `max` = 2 * threshold - 1 - remaining, which grows by what has been spent:
    after k symbols of 1 it is k - 2, so small counts soon take the short
    form.  Candidates: all ones and one big symbol at either end, and a front
    of counts that keep ahead of `max` for as long as 2^14 allows.  The
    longest of them is the case (test_caller_cases.py holds its length)."""
    from oracle import spec

    cands = []
    cands.append([1] * 255 + [(1 << 15) - 255])
    cands.append([(1 << 15) - 255] + [1] * 255)
    cands.append([-1] * 255 + [(1 << 15) - 255])
    front, spent = [], 0
    while True:  # each count >= max - 1 = spent - 3 keeps the long form; stop before remaining < 2^14
        v = max(1, spent - 2)
        if spent + v + (255 - len(front)) > (1 << 14):
            break
        front.append(v)
        spent += v
    tail = [1] * (255 - len(front))
    cands.append(front + tail + [(1 << 15) - spent - len(tail)])
    cands.append(front + tail[:-1] + [(1 << 15) - spent - len(tail)] + [1])
    best = max(cands, key=lambda t: len(spec.header_write(t, 15, 256)))
    assert len(best) == 256 and sum(abs(v) for v in best) == 1 << 15
    return best


def _build_table_cases():
    T = []
    T.append(("all_low_32_L5", [-1] * 32 + [0] * 224))        # every symbol -1; log 5 < ilog2(31) + 2
    T.append(("all_low_256_L8", [-1] * 256))                  # the same at table_len 256, log 8 < 9
    T.append(("ones_256_L8", [1] * 256))                      # log below ilog2(table_len - 1) + 2
    T.append(("ones_64_L6", _table({4 * k: 1 for k in range(64)})))
    T.append(("big_and_low_L5", _table({0: 31, 1: -1})))      # 2^L - 1 beside -1
    T.append(("low_and_big_L15", _table({3: -1, 200: (1 << 15) - 1})))
    T.append(("half_L6", _table({0: 32, 1: 31, 2: 1})))       # 2^(L-1) exactly: fast_mode off
    T.append(("half_minus_one_L6", _table({0: 31, 1: 31, 2: 2})))  # 2^(L-1) - 1: fast_mode on
    T.append(("half_L12", _table({10: 2048, 11: 2047, 255: -1})))
    T.append(("half_minus_one_L12", _table({10: 2047, 11: 2047, 12: 1, 255: -1})))
    runs = [1, 2, 3, 4, 23, 24, 25, 27, 48, 51]
    T.append(("zero_runs_L5", _runs_table(runs, 22, [1] * 10)))
    T.append(("zero_runs_low_L9", _runs_table(runs, 300, [-1, 2, -1, 100, 1, -1, 50, 20, -1, 512 - 477])))
    T.append(("zero_run_253_L5", _table({0: 31, 254: 1})))
    T.append(("zero_run_253_low_L11", _table({0: 2047, 254: -1})))
    T.append(("zero_run_254_L5", _table({0: 16, 255: 16})))   # one 16-bit... 253 repeats: ten 0xFFFF, four 3s, a 1
    T.append(("longest_header_L15", _longest_header()))
    # A last entry of -1 is a 1-bit field read with a 2-bit peek; these headers
    # end on a byte boundary, so without a byte behind them only the
    # peek(read_bit_count - 1) fallback of histogram.rs:471-473 parses them
    T.append(("fallback_L5", _table({0: 1, 1: 30, 2: -1})))
    T.append(("fallback_gap_L5", _table({0: 17, 1: 12, 7: -1, 8: -1, 9: -1})))
    T.append(("fallback_L9", _table({0: 300, 1: 208, 3: -1, 4: -1, 5: -1, 6: -1})))
    return T


TABLE_CASES = _build_table_cases()

# The `remaining <= 1` break of NormHistogram::write (histogram.rs:388-390)
# fires only when the counts reach 2^L before table_len ends.  TryFrom and
# NormHistogram::read both put table_len right behind the last non-zero
# entry, so no TABLE_CASE can reach it; a caller's struct can, with a
# table_len beyond that: (name, table, table_len).
STRUCT_CASES = [
    ("break_before_table_len_L5", _table({0: 16, 3: 16}), 9),
    ("break_before_table_len_L9", _table({0: 500, 1: -1, 40: 11}), 256),
]


# ---------------------------------------------------------------- streams against the table cases
STREAM_LENGTHS = [2, 3, 64, 4097]
STREAM_CAP = 8192  # the output bound every reference-mode decode of these streams gets


def table_alphabet(table):
    return [s for s in range(256) if table[s] != 0]


_streams = None


def table_streams():
    """What the crate's Encoder writes against each table case of two or more
    symbols: NormHistogram::write's header followed by the payload of a
    message over the table's alphabet (tests/shared_ref.compress_shared with
    the image's log limit lifted), in both formats.  A list of dicts: name,
    nstates, n, log, message, stream (None with `status` where the crate's
    Encoder panics, e.g. ENCODER_INIT at log 15), and the oracle's
    reference-mode decode within STREAM_CAP bytes as `want` (bytes or a
    status name).  Built once and shared, read-only."""
    global _streams
    if _streams is not None:
        return _streams
    import shared_ref as R
    from oracle import oracle as O
    from oracle import spec

    out = []
    for ti, (name, table) in enumerate(TABLE_CASES):
        alpha = table_alphabet(table)
        if len(alpha) < 2:
            continue
        norm, L, tl = R.try_from(table)
        head = spec.header_write(norm, L, tl)
        for n in STREAM_LENGTHS:
            rng = random.Random(0x57AB1E + 1000 * ti + n)
            msg = bytes(rng.choice(alpha) for _ in range(n))
            for nstates in (2, 1):
                rec = {"name": name, "nstates": nstates, "n": n, "log": L, "message": msg, "stream": None,
                       "status": None, "want": None}
                try:
                    payload, _ = R.compress_shared(msg, norm, L, tl, nstates, log_max=15)
                except spec.SpecError as e:
                    rec["status"] = e.code
                    out.append(rec)
                    continue
                rec["stream"] = head + payload
                try:
                    rec["want"] = (O.decompress2 if nstates == 2 else O.decompress)(rec["stream"], STREAM_CAP)
                except O.OracleError as e:
                    rec["want"] = e.code
                out.append(rec)
    _streams = out
    return out


def prefix_lengths(n: int):
    """Truncation points of an n-byte header: every prefix up to 64 bytes,
    the last 16 prefix lengths of a longer one (0 is the empty slice), and the
    header itself with no byte behind it."""
    return list(range(0, n + 1)) if n <= 64 else list(range(n - 16, n + 1))
