"""The encoder's top lane: the lane that holds a block's last main-loop steps
has a partial 8-pair (16-symbol, 1-state) chunk whenever the block's step
count is no multiple of the chunk, and for short blocks that lane is lane 0.
Blocks whose step count mod the chunk covers every residue, short blocks and
one 64 KiB block, each encoded alone and as the last of three: the bytes,
payload bits and sidecar must be the oracle's."""
import numpy as np
import pytest

from oracle import oracle as O

gpu = pytest.mark.gpu
CKPT = 64

# 2-state: Pm = n / 2 - 1 (even n), (n - 3) / 2 (odd): 4,096 + {0, 2, ..., 14} has Pm mod 8 = 7, 0, ..., 6;
# the odd lengths + 1 the same Pm with three end symbols
SIZES_2S = [4096 + d for d in range(0, 16)]
# 1-state: Pm = n - 1: Pm mod 16 in {15, 0, 1}
SIZES_1S = [4096, 4097, 4098]
SHORT = [2, 3, 17, 18, 33]  # the top lane is lane 0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def want(x, nstates):
    comp, bits = (O.compress2 if nstates == 2 else O.compress)(x)
    if nstates == 2:
        bp, s0, s1 = O.checkpoints2(comp, CKPT)
        side = bp.astype(np.uint64) | (s0.astype(np.uint64) << 32) | (s1.astype(np.uint64) << 48)
    else:
        bp, s0 = O.checkpoints1(comp, CKPT)
        side = bp.astype(np.uint64) | (s0.astype(np.uint64) << 32)
    return comp, bits, side


def check_blocks(torch, block, blocks, nstates):
    from entropy_coders_amd import BlockCodec

    codec = BlockCodec(block_size=block, ckpt_interval=CKPT, nstates=nstates)
    cb = codec.compress(torch.from_numpy(np.concatenate(blocks)).cuda())
    torch.cuda.synchronize()
    st = cb["status"].tolist()
    bits = cb["payload_bits"].cpu().numpy()
    side = cb["sidecar"].cpu().numpy().view(np.uint64)
    assert st == [0] * len(blocks), (block, nstates, st)
    for b, x in enumerate(blocks):
        tag = (block, nstates, b, len(x))
        comp, wbits, wside = want(x, nstates)
        assert codec.block_bytes(cb, b) == comp, tag
        assert int(bits[b]) & 0xFFFFFFFF == wbits, tag
        mine = side[b * codec.side_per_block: b * codec.side_per_block + len(wside)]
        assert np.array_equal(mine, wside), tag


def data(n, seed):
    return O.generate(0, 0.155, 0x5EED0C00 + seed, 0, n)


@gpu
@pytest.mark.parametrize("nstates,sizes", [(2, SIZES_2S), (1, SIZES_1S)], ids=["2s", "1s"])
def test_partial_top_chunk(torch_cuda, nstates, sizes):
    """One block of every length (a single block may have any size)."""
    for n in sizes:
        check_blocks(torch_cuda, n, [data(n, n)], nstates)


@gpu
@pytest.mark.parametrize("nstates", [2, 1], ids=["2s", "1s"])
def test_partial_top_chunk_last_of_three(torch_cuda, nstates):
    """The same lengths as the short last block of a batch of 4,112-byte blocks."""
    block = 4112
    full = [data(block, 1), data(block, 2)]
    for n in (SIZES_2S if nstates == 2 else SIZES_1S):
        check_blocks(torch_cuda, block, full + [data(n, n)], nstates)


@gpu
@pytest.mark.parametrize("nstates", [2, 1], ids=["2s", "1s"])
def test_top_lane_is_lane_zero(torch_cuda, nstates):
    alpha = np.array([3, 9, 27, 81, 128], dtype=np.uint8)
    rng = np.random.default_rng(0x70C)
    for n in SHORT:
        x = alpha[rng.integers(0, 5, n)]
        x[:2] = [3, 9]  # two symbols at least
        check_blocks(torch_cuda, 4096, [x], nstates)
        check_blocks(torch_cuda, 4096, [data(4096, 3), x], nstates)


@gpu
@pytest.mark.parametrize("nstates", [2, 1], ids=["2s", "1s"])
def test_full_64k_block(torch_cuda, nstates):
    check_blocks(torch_cuda, 65536, [data(65536, 4)], nstates)
