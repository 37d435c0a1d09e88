"""fsehip_copy_blocks, fsehip_pack_blocks and fsehip_unpack_blocks at every
byte alignment and at the lengths where a head or tail byte can be dropped
or a neighbour's byte clobbered (0..9 bytes, either side of 16, longer than
one pass of a workgroup), on synthetic blocks.  The destination is pre-filled
and guarded, the expected buffer is built by numpy slicing into an identical
pre-filled array, and the whole buffer is compared: a neighbour's byte, a gap
byte and a guard byte all count."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_guard_bands import FILL, g8, ptr

gpu = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 255, 1021]
A5 = FILL["uint8"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def copy_layout(rng):
    """(src_off, dst_off, lens) of one fsehip_copy_blocks call: a block for
    every (src_off % 4, dst_off % 4) and every length, destinations apart or
    (a zero gap) touching; then every length three times over with the
    destinations back to back, so neighbours share dwords at every alignment."""
    so, do, ln = [], [], []
    s_cur, d_cur = 0, 0
    for n in LENGTHS:
        for sa in range(4):
            for da in range(4):
                s_cur += int(rng.integers(0, 9))
                s_cur += (sa - s_cur) % 4
                d_cur += int(rng.integers(0, 2)) * 4
                d_cur += (da - d_cur) % 4
                so.append(s_cur)
                do.append(d_cur)
                ln.append(n)
                s_cur += n
                d_cur += n
    d_cur += 1
    for n in rng.permutation(np.repeat(LENGTHS, 3)).tolist():
        s_cur += int(rng.integers(0, 9))
        so.append(s_cur)
        do.append(d_cur)  # back to back
        ln.append(n)
        s_cur += n
        d_cur += n
    order = rng.permutation(len(ln))  # the call's block order is not the layout's
    so, do, ln = (np.asarray(x, dtype=np.int64)[order] for x in (so, do, ln))
    return so, do, ln.astype(np.int32), s_cur, d_cur


@gpu
@pytest.mark.parametrize("dst_skew", range(4))
@pytest.mark.parametrize("src_skew", range(4))
def test_copy_blocks_every_alignment(torch_cuda, src_skew, dst_skew):
    """d_src / d_dst themselves 0..3 bytes off a 4-byte boundary (the header
    allows any alignment of the bases as of the offsets)."""
    torch = torch_cuda
    from entropy_coders_amd import load

    rng = np.random.default_rng(0xC0B1)
    so, do, ln, s_end, d_end = copy_layout(rng)
    both = {(int(s + src_skew) % 4, int(d + dst_skew) % 4) for s, d, n in zip(so, do, ln) if n == 5}
    assert len(both) == 16
    src_host = rng.integers(0, 256, src_skew + s_end, dtype=np.uint8)
    src_host[src_host == A5] = 0x5A  # no source byte looks like the fill
    w_src, src = g8(torch, len(src_host))  # guarded: the kernel's whole-dword reads stay inside the allocation
    src.copy_(_dev(torch, src_host))
    w_dst, dst = g8(torch, dst_skew + d_end)
    want = w_dst.cpu().numpy().copy()
    base = dst.storage_offset() + dst_skew
    for s, d, n in zip(so.tolist(), do.tolist(), ln.tolist()):
        want[base + d: base + d + n] = src_host[src_skew + s: src_skew + s + n]
    d_so, d_do, d_ln = _dev(torch, so), _dev(torch, do), _dev(torch, ln)
    rc = load().fsehip_copy_blocks(C.c_void_p(src.data_ptr() + src_skew), ptr(d_so), ptr(d_ln), len(ln),
                                   C.c_void_p(dst.data_ptr() + dst_skew), ptr(d_do), _stream(torch))
    assert rc == 0
    torch.cuda.synchronize()
    got = w_dst.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), (bad[:8] - base).tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


@gpu
def test_copy_blocks_none(torch_cuda):
    torch = torch_cuda
    from entropy_coders_amd import load

    w_dst, dst = g8(torch, 64)
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    ln = torch.full((1,), 64, dtype=torch.int32, device="cuda")
    assert load().fsehip_copy_blocks(ptr(src), ptr(off), ptr(ln), 0, ptr(dst), ptr(off), _stream(torch)) == 0
    torch.cuda.synchronize()
    assert bool((w_dst == A5).all())


SLOT = 1024
PACK_LENGTHS = [n for n in LENGTHS if n <= 1020] + [1019, 1020, 1022, 1023, 1024]


def pack_case(rng):
    """Slot contents and lengths: every length three times over in random
    order, 0-length blocks in the middle and at both ends, a full slot last
    but one (its last dword is the last of the slot area but for an empty
    slot)."""
    lens = [0] + rng.permutation(np.repeat(PACK_LENGTHS, 3)).tolist() + [SLOT, 0]
    lens = np.asarray(lens, dtype=np.int32)
    assert (lens[1:-1] == 0).any()
    offs = np.cumsum(lens.astype(np.int64)) - lens
    assert {int(o) % 4 for o, n in zip(offs, lens) if n} == {0, 1, 2, 3}
    slots = rng.integers(0, 256, len(lens) * SLOT, dtype=np.uint8)
    slots[slots == A5] = 0x5A
    return slots, lens, offs


@gpu
def test_pack_blocks_every_alignment(torch_cuda):
    torch = torch_cuda
    from entropy_coders_amd import load
    from entropy_coders_amd.dist import pack_host

    slots, lens, offs = pack_case(np.random.default_rng(0x9AC4))
    total = int(lens.sum())
    ref, roffs = pack_host(torch.from_numpy(slots), SLOT, torch.from_numpy(lens))
    assert roffs.tolist() == offs.tolist() and ref.numel() == total
    w_slots, d_slots = g8(torch, len(slots))  # exactly the slot area: the last slot is full
    d_slots.copy_(_dev(torch, slots))
    w_out, out = g8(torch, total)
    want = w_out.cpu().numpy().copy()
    want[out.storage_offset(): out.storage_offset() + total] = ref.numpy()
    d_len, d_off = _dev(torch, lens), _dev(torch, offs)
    rc = load().fsehip_pack_blocks(ptr(d_slots), SLOT, ptr(d_len), ptr(d_off), len(lens), ptr(out), _stream(torch))
    assert rc == 0
    torch.cuda.synchronize()
    got = w_out.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), (bad[:8] - out.storage_offset()).tolist())
    assert bool((w_slots[: d_slots.storage_offset()] == A5).all())  # (the source's own bands: pack only reads)


@gpu
def test_unpack_blocks_every_alignment(torch_cuda):
    """The first len bytes of each slot are the block; the rest of the slot
    keeps what it held (fsehip.h)."""
    torch = torch_cuda
    from entropy_coders_amd import load

    rng = np.random.default_rng(0x9AC5)
    _, lens, offs = pack_case(rng)
    total = int(lens.sum())
    stream = rng.integers(0, 256, total, dtype=np.uint8)
    stream[stream == A5] = 0x5A
    w_stream, d_stream = g8(torch, total)
    d_stream.copy_(_dev(torch, stream))
    w_slots, d_slots = g8(torch, len(lens) * SLOT)
    want = w_slots.cpu().numpy().copy()
    base = d_slots.storage_offset()
    for b, (o, n) in enumerate(zip(offs.tolist(), lens.tolist())):
        want[base + b * SLOT: base + b * SLOT + n] = stream[o: o + n]
    d_len, d_off = _dev(torch, lens), _dev(torch, offs)
    rc = load().fsehip_unpack_blocks(ptr(d_stream), ptr(d_off), ptr(d_len), len(lens), ptr(d_slots), SLOT,
                                     _stream(torch))
    assert rc == 0
    torch.cuda.synchronize()
    got = w_slots.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), (bad[:8] - base).tolist())


def test_pack_copy_call_level():
    """No blocks: FSE_OK with nothing touched, before any device use; null
    pointers and a slot size that is no multiple of 16 are BAD_ARG."""
    from entropy_coders_amd import load

    lib = load()
    a, b, c, d, e = (C.c_void_p(x) for x in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000))  # never dereferenced
    assert lib.fsehip_copy_blocks(a, b, c, 0, d, e, None) == 0
    assert lib.fsehip_pack_blocks(a, SLOT, b, c, 0, d, None) == 0
    assert lib.fsehip_unpack_blocks(a, b, c, 0, d, SLOT, None) == 0
    assert lib.fsehip_copy_blocks(None, b, c, 3, d, e, None) == -11
    assert lib.fsehip_copy_blocks(a, b, c, 3, None, e, None) == -11
    assert lib.fsehip_pack_blocks(a, SLOT + 8, b, c, 3, d, None) == -11
    assert lib.fsehip_unpack_blocks(a, b, None, 3, d, SLOT, None) == -11
