"""Reference for shared-table coding (include/fsehip.h section 2c), pure
Python: oracle/spec.py's encode_table, _Enc, BitSink, decode_table and Stack
composed into the payload of a message against a caller's table, and the two
decode modes.  With the message's own normalised histogram as the table the
payload is the oracle's stream minus its header (tests/test_shared_table_ref.py
pins that), so everything here hangs on the C oracle through spec.py.

Statuses are raised as spec.SpecError(code), in the order the header gives.
"""
from __future__ import annotations

from functools import lru_cache

from oracle import spec
from oracle.spec import SpecError

MAX_SRC = 65536
LOG_MAX_SHARED = 12


class Sink(spec.BitSink):
    """BitSink with the bits packed as they come (a 65,536-byte message is
    700,000 bits: a list of them is too slow to share among the GPU tests)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.nbits = 0

    def put(self, val: int, n: int) -> None:
        self.acc |= (val & ((1 << n) - 1)) << self.n
        self.n += n
        self.nbits += n
        if self.n >= 64:
            self.out += (self.acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            self.acc >>= 64
            self.n -= 64

    def to_bytes(self) -> bytes:
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) // 8, "little")


def try_from(table):
    """`impl TryFrom<[i32; 256]> for NormHistogram` (histogram.rs:508-536) ->
    (norm, log2, table_len); Err(()) and the 0.ilog2() panic are BAD_TABLE."""
    assert len(table) == 256
    total = sum(abs(int(x)) for x in table)
    if total == 0 or total & (total - 1):
        raise SpecError("BAD_TABLE")
    nz = [i for i, x in enumerate(table) if x]
    return [int(x) for x in table], total.bit_length() - 1, nz[-1] + 1


def build_status(norm, L, table_len, log_max: int = LOG_MAX_SHARED) -> str:
    """What fsehip_shared_table_build reports for this NormHistogram
    (log_max = 15: what the crate's EncodeTable::new accepts)."""
    if not spec.LOG_MIN <= L <= spec.LOG_MAX:
        return "TABLELOG_RANGE"
    if L > log_max:
        return "UNSUPPORTED"
    if not 1 <= table_len <= 256:
        return "BAD_TABLE"
    used = norm[:table_len]
    if any(v < -1 for v in used) or sum(1 if v == -1 else v for v in used) != 1 << L:
        return "BAD_TABLE"
    try:
        spec.spread(norm, L, table_len)
    except SpecError as e:
        return e.code
    return "OK"


@lru_cache(maxsize=64)
def _tables(norm: tuple, L: int, table_len: int):
    return spec.encode_table(list(norm), L, table_len), spec.decode_table(list(norm), L, table_len)


def compress_shared(src: bytes, norm, L: int, table_len: int, nstates: int = 2,
                    log_max: int = LOG_MAX_SHARED) -> tuple[bytes, int]:
    """The payload of `src` against the table and its bit count (marker
    included): lib.rs:151-182 at two states, fse.rs:394-421 at one.  log_max
    = 15 lifts the shared image's limit of 12 (the crate's Encoder has none)."""
    src = bytes(src)
    n = len(src)
    if build_status(norm, L, table_len, log_max) != "OK":
        raise SpecError("BAD_TABLE")
    if n == 0:
        raise SpecError("EMPTY")
    if nstates == 2 and n == 1:
        raise SpecError("TOO_SHORT")
    if n > MAX_SRC:
        raise SpecError("UNSUPPORTED")
    if any(s >= table_len or norm[s] == 0 for s in set(src)):
        raise SpecError("SYMBOL_NOT_IN_TABLE")  # fse.rs:231-238 indexes unchecked
    tab = _tables(tuple(norm), L, table_len)[0]
    sink = Sink()
    if nstates == 2:
        if n % 2:
            e0, e1 = spec._Enc(tab, src[n - 1]), spec._Enc(tab, src[n - 2])
            e0.step(src[n - 3], sink)
            top = (n - 3) // 2
        else:
            e0, e1 = spec._Enc(tab, src[n - 2]), spec._Enc(tab, src[n - 1])
            top = n // 2 - 1
        for k in range(top - 1, -1, -1):
            e1.step(src[2 * k + 1], sink)
            e0.step(src[2 * k], sink)
        e1.finish(L, sink)
        e0.finish(L, sink)
    else:
        chunks = [src[i:i + 2] for i in range(0, n, 2)]
        first = chunks.pop()
        e = spec._Enc(tab, first[-1])
        if len(first) > 1:
            e.step(first[0], sink)
        for ch in reversed(chunks):
            e.step(ch[1], sink)
            e.step(ch[0], sink)
        e.finish(L, sink)
    sink.put(1, 1)
    return sink.to_bytes(), sink.nbits


def decompress_shared(payload: bytes, norm, L: int, table_len: int, nstates: int = 2, raw_len: int | None = None,
                      out_cap: int = 1 << 24) -> bytes:
    """The message of a payload: the crate's loops (lib.rs:222-247 / 187-211)
    with the serial decoders' end rules.  raw_len=None: the crate's own
    termination within out_cap; else the payload must end with raw_len bytes
    (LENGTH_MISMATCH otherwise: the block decoders stop at the raw length
    whatever follows, this one also asks that the payload ends there)."""
    if build_status(norm, L, table_len) != "OK":
        raise SpecError("BAD_TABLE")
    known = raw_len is not None
    lim = raw_len if known else out_cap
    if len(payload) == 0:
        raise SpecError("EMPTY")
    stack = spec.Stack(bytes(payload))  # NO_MARKER
    if lim > out_cap:
        raise SpecError("DST_TOO_SMALL")
    if nstates == 2 and known and lim < 2:
        raise SpecError("LENGTH_MISMATCH")
    single = spec._single_symbol(norm[:table_len], L)
    if not known and single:
        raise SpecError("SINGLE_SYMBOL")
    dt = _tables(tuple(norm), L, table_len)[1]
    states = [stack.pop(L) for _ in range(nstates)] if len(stack.bits) >= nstates * L else None
    if states is None:
        raise SpecError("TOO_SHORT")
    out = bytearray()
    full = "LENGTH_MISMATCH" if known else "DST_TOO_SMALL"

    def step(state):
        ns, _, nb = dt[state]
        b = stack.pop(nb)
        return None if b is None else (ns + b) & 0xFFFF

    def sym(state):
        return dt[state][1]

    if nstates == 2:
        s0, s1 = states
        nb1 = 0  # bits of decoder 1's last read
        while True:
            if known and len(out) + 2 >= lim:
                # the payload must end here too: no bit left, and where one byte is missing decoder 1's last read
                # took none (a read that took bits undid a step of the encoder: the message is longer)
                if stack.bits or (len(out) + 2 != lim and nb1):
                    raise SpecError("LENGTH_MISMATCH")
                out += bytes([sym(s0), sym(s1)][: lim - len(out)])
                break
            for a in (0, 1):
                cur, other = (s0, s1) if a == 0 else (s1, s0)
                y, nxt = sym(cur), step(cur)
                if a == 1:
                    nb1 = dt[cur][2]
                if nxt is None:
                    if len(out) + 2 > lim:
                        raise SpecError(full)
                    out += bytes([y, sym(other)])
                    break
                if len(out) >= lim:
                    raise SpecError(full)
                out.append(y)
                if a == 0:
                    s0 = nxt
                else:
                    s1 = nxt
            else:
                continue
            break
        if known and len(out) != lim:
            raise SpecError("LENGTH_MISMATCH")
    else:
        st = states[0]
        while True:
            if known and single and len(out) + 1 >= lim:
                break
            y, nxt = sym(st), step(st)
            if nxt is None:
                break
            if len(out) >= lim:
                raise SpecError(full)
            out.append(y)
            st = nxt
        if len(out) >= lim:
            raise SpecError(full)
        out.append(sym(st))
        if known and len(out) != lim:
            raise SpecError("LENGTH_MISMATCH")
    return bytes(out)


def train(samples, table_log: int = 11, floor: int = 1):
    """The histogram of the samples plus `floor` on all 256 symbols, through
    Histogram::normalize(table_log) -> (norm, L, table_len)."""
    counts = [floor] * 256
    for s in samples:
        for b in bytes(s):
            counts[b] += 1
    size = sum(counts)
    table_len = max(i for i in range(256) if counts[i]) + 1
    norm, L, _ = spec.normalize(counts, size, table_len, table_log)
    return norm, L, table_len
