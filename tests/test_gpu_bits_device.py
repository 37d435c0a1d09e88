"""The device bit primitives (fsehip_bitstack_write, fsehip_bitstack_read,
fsehip_bitstream_read_ops) on device tensors, across tiles (4,096 fields)
and across the 1,024-tile chunks of the tile scan, with the first failing
step placed by construction, against a vectorised numpy model that is
itself checked on the CPU against oracle.spec and the oracle's writer and
stack reader.  Outputs sit between guard bands (test_gpu_guard_bands)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from oracle import spec
from test_gpu_guard_bands import FILL, assert_all_written, assert_guards, g8, g32, g64, ptr

gpu = pytest.mark.gpu

READ, PEEK, ADVANCE = 0, 1, 2  # FSE_BITS_* (include/fsehip.h)
TILE = 4096  # fields per workgroup of the bit kernels; the tile scan takes 1,024 tiles per chunk
NO_MARKER, BAD_ARG = -6, -11
BIG = 4_300_000  # 1,050 tiles: the scan's second chunk runs, with a carry


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ---------------------------------------------------------------- the model
def model_positions(widths, ops, available):
    """(clamped widths, position of every step, first failing step or count).
    Positions are the exclusive running sum of the advances (a peek advances
    0, widths are clamped to 32); a step fails when pos + width > available."""
    w = np.minimum(np.asarray(widths, dtype=np.int64), 32)
    adv = w.copy()
    if ops is not None:
        adv[np.asarray(ops) == PEEK] = 0
    pos = np.cumsum(adv) - adv
    fail = pos + w > available
    first = int(np.argmax(fail)) if fail.any() else len(w)
    return w, pos, first


def model_gather(data, lo, w):
    """The w[i] bits from bit lo[i] on of the zero-padded LSB-first stream."""
    pad = np.zeros(len(data) + 8, dtype=np.uint8)
    pad[: len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
    byte = lo >> 3
    x = np.zeros(len(lo), dtype=np.uint64)
    for k in range(5):
        x |= pad[byte + k].astype(np.uint64) << np.uint64(8 * k)
    mask = (np.uint64(1) << w.astype(np.uint64)) - np.uint64(1)
    return ((x >> (lo & 7).astype(np.uint64)) & mask).astype(np.uint32)


def model_stream(data, total_bits, widths, ops=None):
    """BitStreamReader steps: (values of the steps before the first failing
    one, its index, whether the steps consume exactly total_bits)."""
    w, pos, first = model_positions(widths, ops, total_bits)
    vals = model_gather(data, pos[:first], w[:first])
    if ops is not None:
        vals[np.asarray(ops)[:first] == ADVANCE] = 0
    used = int(pos[-1] + (0 if ops is not None and ops[-1] == PEEK else w[-1])) if len(w) else 0
    return vals, first, used == total_bits


def stack_available(data):
    """Bits below the marker (the highest set bit of the last byte), or None."""
    if len(data) == 0 or data[-1] == 0:
        return None
    return 8 * (len(data) - 1) + int(data[-1]).bit_length() - 1


def model_stack(data, widths):
    """BitStackReader reads, top down: field i ends at available - pos_i."""
    av = stack_available(data)
    w, pos, first = model_positions(widths, None, av)
    vals = model_gather(data, av - pos[:first] - w[:first], w[:first])
    used = int(pos[-1] + w[-1]) if len(w) else 0
    return vals, first, used == av


def random_widths(rng, count):
    """Widths 0..32 with many 0-bit and 32-bit fields, and whole runs of 16
    and of a tile of 0-bit fields (threads and a workgroup with a zero total)."""
    w = rng.integers(0, 33, count).astype(np.uint8)
    pick = rng.random(count)
    w[pick < 0.15] = 0
    w[pick > 0.85] = 32
    if count >= 64:
        for start in rng.integers(0, count - 16, max(count // 400, 1)):
            start = int(start) // 16 * 16
            w[start: start + 16] = 0
    if count >= 3 * TILE:
        w[TILE: 2 * TILE] = 0
    return w


def masked(vals, widths):
    w = np.minimum(widths.astype(np.uint64), np.uint64(32))
    return (vals.astype(np.uint64) & ((np.uint64(1) << w) - np.uint64(1))).astype(np.uint64)


def failing_stream_case(rng, k, tail):
    """A stream and k + 1 + tail reads of which step k is the first to fail:
    the stream holds the first k fields and one bit less than field k."""
    count = k + 1 + tail
    widths = random_widths(rng, count)
    widths[k] = 9
    vals = masked(rng.integers(0, 1 << 32, k + 1, dtype=np.uint64), np.append(widths[:k], 8))
    data, total = O.bits_write(vals, np.append(widths[:k], 8).astype(np.uint8), False)
    return data, total, widths


def failing_stack_case(rng, k, tail):
    """A stack and k + 1 + tail reads of which read k is the first to fail:
    below the marker lie, bottom up, 8 bits and the first k fields reversed."""
    count = k + 1 + tail
    widths = random_widths(rng, count)
    widths[k] = 9
    wr = np.append(8, widths[:k][::-1]).astype(np.uint8)
    vals = masked(rng.integers(0, 1 << 32, k + 1, dtype=np.uint64), wr)
    data, bits = O.bits_write(vals, wr, True)
    assert stack_available(data) == bits
    return data, widths, vals[1:][::-1].astype(np.uint32)


FAIL_AT = [(0, 5000), (TILE - 1, 5000), (TILE, 5000), (3 * TILE + 4, 0)]  # (first failing step, steps after it)


def test_model_on_cpu():
    """The numpy model against oracle.spec.stream_steps (reads, peeks and
    advances, running past the end), the oracle's writer and its stack
    reader; then the failing-step constructions the GPU tests use."""
    rng = np.random.default_rng(0xB175)
    # 20,000 random steps over a stream they overrun near the end
    count = 20000
    widths = rng.integers(0, 33, count).astype(np.uint8)
    ops = rng.integers(0, 3, count).astype(np.uint8)
    _, pos, _ = model_positions(widths, ops, 1 << 62)
    total = int(pos[count - 40])  # the steps run past it there, or at a peek shortly before
    long = rng.integers(0, 256, (total + 32 + 7) // 8, dtype=np.uint8).tobytes()
    data = long[: (total + 7) // 8]
    vals, first, fin = model_stream(data, total, widths, ops)
    want = spec.stream_steps(data, total, widths.tolist(), ops.tolist())
    assert count - 100 < first < count and not fin
    assert first == want[1] and vals.tolist() == want[0]
    # 32 bits more: every step up to there succeeds
    w2, o2 = widths[: count - 40], ops[: count - 40]
    vals, first, fin = model_stream(long, total + 32, w2, o2)
    want = spec.stream_steps(long, total + 32, w2.tolist(), o2.tolist())
    assert first == want[1] == len(w2) and vals.tolist() == want[0] and want[2] == 32 and not fin
    # the writer, and the stack read back: wide fields through the model, <= 16 bits also through the oracle's reader
    for hi in (17, 33):
        widths = rng.integers(0, hi, count).astype(np.uint8)
        vals = masked(rng.integers(0, 1 << 32, count, dtype=np.uint64), widths)
        data, bits = O.bits_write(vals, widths, True)
        assert stack_available(data) == bits == int(widths.sum())
        got, first, fin = model_stack(data, widths[::-1])
        assert first == count and fin and np.array_equal(got, vals[::-1].astype(np.uint32))
        if hi == 17:
            ref, left = O.bits_read_stack(data, widths)
            assert left == 0 and ref == vals.tolist()
        got, first, fin = model_stack(data, np.append(widths[::-1], 1))  # one read too many
        assert first == count and not fin
        fwd, total = O.bits_write(vals, widths, False)
        got, first, fin = model_stream(fwd, total, widths)
        assert first == count and fin and np.array_equal(got, vals.astype(np.uint32))
    assert stack_available(b"") is None and stack_available(b"\x12\x00") is None
    # the failing-step constructions
    for k, tail in FAIL_AT:
        data, total, widths = failing_stream_case(rng, k, tail)
        vals, first, fin = model_stream(data, total, widths)
        want = spec.stream_steps(data, total, widths.tolist(), [0] * len(widths))
        assert first == k == want[1] and vals.tolist() == want[0] and not fin
        data, widths, expect = failing_stack_case(rng, k, tail)
        vals, first, fin = model_stack(data, widths)
        assert first == k and not fin and np.array_equal(vals, expect)


def test_bitstream_read_ops_bad_args():
    """BitStreamReader::new's asserts (n == ceil(total_bits / 8) > 0) as
    BAD_ARG, returned before any device use (no GPU needed)."""
    from entropy_coders_amd import load

    lib = load()
    a, b, c, d, e = (C.c_void_p(x) for x in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000))  # never dereferenced
    for n_bytes, total in ((2, 20), (4, 20), (0, 0), (0, 8), (3, 25)):
        assert lib.fsehip_bitstream_read_ops(a, n_bytes, total, b, c, 4, d, e, None) == BAD_ARG, (n_bytes, total)
        assert lib.fsehip_bitstream_read(a, n_bytes, total, b, 4, d, e, None) == BAD_ARG, (n_bytes, total)


# ---------------------------------------------------------------- device calls
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_stream(torch, data):
    """The stream's bytes on the device, readable up to roundup(n, 4) (zeros)."""
    a = np.zeros((len(data) + 3) // 4 * 4 + 4, dtype=np.uint8)
    a[: len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
    return _dev(torch, a)


def _read(torch, lib, reader, data, total, widths, ops=None):
    """One device read call into guarded d_vals / d_result: (vals, result)."""
    count = len(widths)
    d_in = _dev_stream(torch, data)
    d_w = _dev(torch, widths.astype(np.uint8))
    d_ops = _dev(torch, ops.astype(np.uint8)) if ops is not None else None
    w_v, vals = g32(torch, count)
    w_r, res = g64(torch, 3)
    hs = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if reader == "stack":
        rc = lib.fsehip_bitstack_read(ptr(d_in), len(data), ptr(d_w), count, ptr(vals), ptr(res), hs)
    else:
        rc = lib.fsehip_bitstream_read_ops(ptr(d_in), len(data), total, ptr(d_w), ptr(d_ops) if ops is not None else
                                           None, count, ptr(vals), ptr(res), hs)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guards(w_v, vals, FILL["int32"], f"{reader} d_vals")
    assert_guards(w_r, res, FILL["int64"], f"{reader} d_result")
    assert_all_written(res, FILL["int64"], f"{reader} d_result")
    return vals.cpu().numpy().view(np.uint32), res.tolist()


@gpu
@pytest.mark.parametrize("count", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, BIG])
def test_bitstack_write_then_stack_read(torch_cuda, count):
    """fsehip_bitstack_write of `count` fields and the marker bit equals the
    oracle's writer byte for byte, inside a d_out of exactly the capacity the
    header asks for; fsehip_bitstack_read gives the fields back, top down."""
    torch = torch_cuda
    from entropy_coders_amd import load

    lib = load()
    rng = np.random.default_rng(0x57AC + count)
    widths = random_widths(rng, count)
    vals = rng.integers(0, 1 << 32, count, dtype=np.uint64)
    m = masked(vals, widths)
    want, wbits = O.bits_write(m, widths, True)
    total = wbits + 1
    assert len(want) == (total + 7) // 8
    if count >= TILE:
        assert (widths == 0).sum() > count // 16 and (widths == 32).sum() > count // 16
    cap = 4 * ((total + 31) // 32)
    d_v = _dev(torch, np.append(vals, 1).astype(np.uint32).view(np.int32))  # unmasked: the writer masks
    d_w = _dev(torch, np.append(widths, 1).astype(np.uint8))
    w_o, d_out = g8(torch, cap)
    w_t, d_tot = g64(torch, 1)
    hs = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.fsehip_bitstack_write(ptr(d_v), ptr(d_w), count + 1, ptr(d_out), cap, ptr(d_tot), hs) == 0
    torch.cuda.synchronize()
    assert_guards(w_o, d_out, FILL["uint8"], "d_out")
    assert_guards(w_t, d_tot, FILL["int64"], "d_total_bits")
    assert d_tot.tolist() == [total]
    assert d_out[: len(want)].cpu().numpy().tobytes() == want
    got, res = _read(torch, lib, "stack", want, 0, widths[::-1])
    assert res == [count, 1, 0]
    assert np.array_equal(got, m[::-1].astype(np.uint32))


@gpu
@pytest.mark.parametrize("k,tail", FAIL_AT)
@pytest.mark.parametrize("reader", ["stack", "stream"])
def test_first_failing_step(torch_cuda, reader, k, tail):
    """One read too many at step k, and `tail` further (failing) steps in
    later tiles: result[0] is the earliest failing index, not finished, and
    the values before it are exact."""
    torch = torch_cuda
    from entropy_coders_amd import load

    rng = np.random.default_rng(0xFA11 + k)
    if reader == "stack":
        data, widths, _ = failing_stack_case(rng, k, tail)
        total = 0
        want, first, fin = model_stack(data, widths)
    else:
        data, total, widths = failing_stream_case(rng, k, tail)
        want, first, fin = model_stream(data, total, widths)
    assert first == k and not fin
    got, res = _read(torch, load(), reader, data, total, widths)
    assert res == [k, 0, 0]
    assert np.array_equal(got[:k], want)


@gpu
def test_stack_without_marker(torch_cuda):
    torch = torch_cuda
    from entropy_coders_amd import load

    widths = np.full(10, 3, dtype=np.uint8)
    for data in (b"\x12\x34\x00", b""):
        _, res = _read(torch, load(), "stack", data, 0, widths)
        assert res == [0, 0, NO_MARKER]


@gpu
@pytest.mark.parametrize("count", [TILE + 1, BIG])
def test_bitstream_read_ops_device(torch_cuda, count):
    """Random reads, peeks and advances with the ops on the device, and a
    three-step tail that runs past total_bits, against the model."""
    torch = torch_cuda
    from entropy_coders_amd import load

    rng = np.random.default_rng(0x0B5 + count)
    widths = random_widths(rng, count)
    ops = rng.integers(0, 3, count).astype(np.uint8)
    _, pos, _ = model_positions(np.append(widths, 0), np.append(ops, READ), 1 << 62)
    total = int(pos[-1]) + 36  # 36 bits beyond the body's: its peeks fit as well
    widths = np.append(widths, [32, 32, 16]).astype(np.uint8)
    ops = np.append(ops, [PEEK, ADVANCE, READ]).astype(np.uint8)  # a peek and an advance that fit, a read that does not
    data = rng.integers(0, 256, (total + 7) // 8, dtype=np.uint8).tobytes()
    want, first, fin = model_stream(data, total, widths, ops)
    assert first == count + 2 and not fin
    got, res = _read(torch, load(), "stream", data, total, widths, ops)
    assert res == [first, 0, 0]
    assert np.array_equal(got[:first], want)
