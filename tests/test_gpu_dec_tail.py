"""The segment decoder's partial last group: the pairs (2-state) or symbols
(1-state) a segment has beyond its whole 64-byte groups are decoded inside the
wave-synchronous group loop, each predicated on the lane's own count, and
stored by their owner lane.  Every case is a batch whose short last block
comes from n_total; the blocks' bytes are compared with the oracle, the decode
must be exact with every status 0, and a guard band after `out` must stay as
it was (no store at or past a block's end: the next bytes belong to another
workgroup, or to nobody)."""
import numpy as np
import pytest

from oracle import oracle as O

gpu = pytest.mark.gpu

GUARD = 256
FILL = 0xA5

# last-block lengths: Pm mod 32 in {0, 1, 30, 31} (2-state; Pm = pairs before
# the end symbols), even and odd n, a last segment that is only the end
# symbols (130, 131 at 64-pair checkpoints), and one pair short of a block
LAST = [2, 3, 4, 5, 64, 65, 66, 67, 126, 127, 128, 129, 130, 131, 190, 191, 192, 193, 4095]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def guarded_out(torch, n):
    """(whole, view): n bytes that start 256-byte aligned with GUARD bytes of FILL behind them."""
    body = (n + GUARD - 1) // GUARD * GUARD
    whole = torch.full((body + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % GUARD == 0
    return whole, whole[:n]


def round_trip(torch, block, n_total, nstates, ckpt, data=(0, 0.155), seed=0x5EED0A00, oracle_blocks=(0, -1)):
    """Encode n_total bytes, check blocks against the oracle, decode into a
    guarded buffer: exact, every status 0, guard untouched.  Returns what a
    damaged-sidecar case needs."""
    from entropy_coders_amd import BlockCodec

    what = f"block {block} n_total {n_total} nstates {nstates} ckpt {ckpt} data {data}"
    codec = BlockCodec(block_size=block, ckpt_interval=ckpt, nstates=nstates)
    nb = codec.n_blocks(n_total)
    assert 8 <= nb <= 64, what
    src = codec.generate(data[0], data[1], seed + block + n_total, n_total)
    cb = codec.compress(src)
    torch.cuda.synchronize()
    assert cb["status"].tolist() == [0] * nb, what
    host = src.cpu().numpy()
    for b in oracle_blocks:
        b %= nb
        s = host[b * block: min((b + 1) * block, n_total)]
        want, wbits = O.compress2(s) if nstates == 2 else O.compress(s)
        assert codec.block_bytes(cb, b) == want and int(cb["payload_bits"][b]) == wbits, (what, b)
    whole, out = guarded_out(torch, n_total)
    st = torch.full((nb,), -99, dtype=torch.int32, device="cuda")
    codec.decompress_into(cb, out, st)
    torch.cuda.synchronize()
    assert st.tolist() == [0] * nb, (what, st.tolist())
    assert torch.equal(out, src), what
    assert bool((whole[n_total:] == FILL).all()), f"{what}: a store past the last block's end"
    return codec, src, cb


# ---------------------------------------------------------------- 64 KiB blocks, 2-state
@gpu
@pytest.mark.parametrize("ckpt", [64, 128], ids=["ckpt64-512thr", "ckpt128-256thr"])
@pytest.mark.parametrize("last", [65536, 40001, 126])
def test_full_blocks_two_state(torch_cuda, ckpt, last):
    """Full blocks: 32,767 main-loop pairs, so the last segment holds 63 (64-pair
    checkpoints) or 127 (128-pair) and ends on a 31-pair partial group."""
    round_trip(torch_cuda, 65536, 8 * 65536 + last, 2, ckpt)


@gpu
def test_full_blocks_list_pass(torch_cuda):
    """Uniform bytes 0..239: the compressed blocks exceed the first stage and go
    through the list pass (the 66 KiB stage)."""
    codec, _, cb = round_trip(torch_cuda, 65536, 8 * 65536 + 40001, 2, 64, data=(2, 0.0))
    assert int(cb["comp_len"][:8].min()) > 44 * 1024  # above the first pass's stage


# ---------------------------------------------------------------- 4 KiB blocks, every tail shape
@gpu
@pytest.mark.parametrize("ckpt", [64, 128])
@pytest.mark.parametrize("nstates", [2, 1], ids=["2s", "1s"])
def test_last_block_lengths_4k(torch_cuda, nstates, ckpt):
    for last in LAST:
        round_trip(torch_cuda, 4096, 8 * 4096 + last, nstates, ckpt)


@gpu
@pytest.mark.parametrize("ckpt", [64, 128])
def test_last_block_lengths_64k_one_state(torch_cuda, ckpt):
    """1-state, 64 KiB blocks: 1,024 or 512 segments (the 512-thread kernel, two
    rounds or one), the last one 63 or 127 symbols."""
    for last in LAST:
        round_trip(torch_cuda, 65536, 8 * 65536 + last, 1, ckpt, oracle_blocks=(-1,))


@gpu
@pytest.mark.parametrize("ckpt", [8, 16, 32])
def test_checkpoints_closer_than_a_group(torch_cuda, ckpt):
    """Checkpoints every 8, 16 or 32 pairs: every segment is at most one group,
    and below 32 every segment is a partial one (1-state: 16 and 32 symbols)."""
    for last in (5, 67, 191, 4095):
        round_trip(torch_cuda, 4096, 8 * 4096 + last, 2, ckpt)
        if ckpt >= 16:
            round_trip(torch_cuda, 4096, 8 * 4096 + last, 1, ckpt)


# ---------------------------------------------------------------- damaged sidecar
@gpu
@pytest.mark.parametrize("which", ["last", "before-last"])
@pytest.mark.parametrize("victim", [3, 8], ids=["middle-block", "short-last-block"])
def test_damaged_sidecar_entry(torch_cuda, victim, which):
    """A damaged entry of the last segment (its bit position past the block:
    the segment is not decoded) or of the one before it (a flipped state bit:
    the segment two before fails its cross-check): the block's status is
    BAD_SIDECAR, every other block decodes exactly, and nothing is written
    past the output (the victim is the batch's short last block in one case)."""
    torch = torch_cuda
    from entropy_coders_amd._lib import STATUS

    block, ckpt, last = 65536, 64, 40001
    n_total = 8 * block + last
    codec, src, cb = round_trip(torch, block, n_total, 2, ckpt, oracle_blocks=())
    nb = codec.n_blocks(n_total)
    n = block if victim < nb - 1 else last
    pm = (n - 3) // 2 if n & 1 else n // 2 - 1
    nseg = pm // ckpt + 1
    assert nseg >= 3 and pm % ckpt  # the last segment has pairs of its own
    side = cb["sidecar"].clone()
    e = victim * codec.side_per_block + nseg - 1
    if which == "last":
        side[e] = (int(side[e]) & ~0xFFFFFFFF) | 0x7FFFFFF0
    else:
        side[e - 1] = int(side[e - 1]) ^ (1 << 32)
    bad = dict(cb, sidecar=side)
    whole, out = guarded_out(torch, n_total)
    st = torch.full((nb,), -99, dtype=torch.int32, device="cuda")
    codec.decompress_into(bad, out, st)
    torch.cuda.synchronize()
    status = st.tolist()
    assert STATUS[status[victim]] == "BAD_SIDECAR", status
    assert [s for b, s in enumerate(status) if b != victim] == [0] * (nb - 1), status
    assert bool((whole[n_total:] == FILL).all()), "a store past the last block's end"
    for b in range(nb):
        if b != victim:
            lo, hi = b * block, min((b + 1) * block, n_total)
            assert torch.equal(out[lo:hi], src[lo:hi]), b
