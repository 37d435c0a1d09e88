"""References for containers past 4 GiB: a helper for tests/test_large_ref.py
and tests/test_gpu_large.py, not a test.

A frame's record for a block follows from that block's bytes and length
alone (its FSE bytes, its block-relative checkpoints, its RAW / RLE
fallback).  So a source that is one tile of TILE_BLOCKS whole blocks repeated
k times and then a ragged tail has the frame

    header(n_total) | (tile directory x k | tail entry) | (tile records x k | tail record)

whose pieces come from tests/frame_ref.build_frame on the CPU oracle over 15 +
1 blocks.  The repeats are laid out with tensor ops on whatever device is
asked for, so the expected frame of a 4 GiB+ source costs milliseconds and
reads nothing from the library under test.

  tile_and_tail    the numpy tile and tail, with the tile's requirements asserted
  tiled_source     the source tensor
  tiled_layout     the pieces of the expected frame and its lengths
  tiles_for        the smallest k whose reference frame passes a given length
  tiled_frame      the expected frame as a tensor
  block_of_frame_offset  the block whose record holds a frame offset; record_span: the inverse
  tiled_crc32, tiled_crc   zlib.crc32 of the tiled content by combines; its check record
  tiled_estimate   estimate_ref's frame estimate of the tiled content
  planes_image, planes_unimage, delta_image, diff_image
                   planes_ref / delta_ref / diff_ref images restated as torch ops

Nothing here calls the library under test.
"""
import zlib

import numpy as np
import torch

import check_ref as CR
import delta_ref as DR
import estimate_ref as E
import frame_ref as R
import planes_ref as PR
from oracle import oracle as O

# 2^32 bytes are 65,536 blocks of 64 KiB and 65,536 mod 15 = 1; 2^31 bytes are
# 32,768 blocks and 32,768 mod 15 = 8.  An offset that wrapped by 2^32 or 2^31
# therefore lands on a DIFFERENT block of the tile, and the blocks of the tile
# all differ.  A tile of 16 or 32 blocks divides both and would make every
# such wrap invisible: the wrapped offset would find the very bytes it expects.
TILE_BLOCKS = 15
BLOCK = 65536
TAIL = 40001
WRAPS = (1 << 32, 1 << 31)

RLE_AT = 7          # the all-zero block: one, in the middle, so never next to itself across the tile seam
FSE_AT = (3, 11)    # the two LUT blocks; the twelve others are uniform random bytes


def check_tile_blocks(t, block_size):
    """The tile size's own requirement: no wrap of WRAPS is a whole number of tiles."""
    for wrap in WRAPS:
        assert wrap % block_size == 0, (wrap, block_size)
        assert (wrap // block_size) % t != 0, f"a tile of {t} blocks hides an offset wrapped by {wrap}"


def tile_and_tail(seed, block_size=BLOCK, tail_len=TAIL, tile_blocks=TILE_BLOCKS):
    """(tile, tail): uint8 arrays of tile_blocks * block_size and tail_len bytes."""
    check_tile_blocks(tile_blocks, block_size)
    assert tile_blocks == TILE_BLOCKS  # RLE_AT and FSE_AT are places in a tile of 15
    assert 0 < tail_len < block_size and tail_len % 2 == 1
    rng = np.random.default_rng(seed)
    blocks = []
    for b in range(tile_blocks):
        if b == RLE_AT:
            blocks.append(np.zeros(block_size, dtype=np.uint8))
        elif b in FSE_AT:
            blocks.append(O.generate(0, 0.155, (seed + 0x5EED) & 0x7FFFFFFF, b, block_size))
        else:
            blocks.append(rng.integers(0, 256, block_size, dtype=np.uint8))
    tail = O.generate(0, 0.155, (seed + 0x7A11) & 0x7FFFFFFF, tile_blocks, tail_len)
    for i in range(tile_blocks):
        assert len(blocks[i]) == block_size
        # no single-symbol block but the zero one: frame_ref.oracle_checkpoints cannot walk one
        assert (np.unique(blocks[i]).size > 1) != (i == RLE_AT), i
        for j in range(i + 1, tile_blocks):  # all pairs, so the cyclic distances 1 and 8 among them
            assert not np.array_equal(blocks[i], blocks[j]), (i, j)
    for d in (1, 8):
        for i in range(tile_blocks):
            assert not np.array_equal(blocks[i], blocks[(i + d) % tile_blocks]), (i, d)
    assert np.unique(tail).size > 1
    return np.concatenate(blocks), np.ascontiguousarray(tail)


def rotated(tile, block_size=BLOCK, by=1):
    """The tile rotated by whole blocks: another tile of the same blocks."""
    return np.roll(tile, by * block_size)


def _tensor(a, device):
    return torch.from_numpy(np.array(a, copy=True)).to(device)


def _fill_repeats(dst, piece, k):
    """dst (k * len(piece) bytes) = piece repeated k times: Tensor.repeat written into its place."""
    assert dst.numel() == k * piece.numel()
    if k and piece.numel():
        dst.view(k, piece.numel()).copy_(piece.unsqueeze(0).expand(k, piece.numel()))


def tiled_source(tile, k, tail, device="cpu"):
    """tile * k + tail as a uint8 tensor on `device`."""
    out = torch.empty(k * len(tile) + len(tail), dtype=torch.uint8, device=device)
    _fill_repeats(out[: k * len(tile)], _tensor(tile, device), k)
    out[k * len(tile):] = _tensor(tail, device)
    return out


def tiled_layout(tile, k, tail, block_size, ckpt, nstates):
    """The pieces of the expected frame, from frame_ref.build_frame of the
    tile and of the tail: a dict with the bytes `header`, `tile_dir`,
    `tail_dir`, `tile_rec`, `tail_rec`; `rec_lens` (the record bytes of each
    tile block), `types` (of each tile block), `tail_type`; `n_total`,
    `n_blocks`, `records_off` and `frame_len`."""
    t = len(tile) // block_size
    assert len(tile) == t * block_size and 0 < len(tail) < block_size
    tf = R.build_frame(tile, block_size, ckpt, nstates)
    lf = R.build_frame(tail, block_size, ckpt, nstates)
    _, tdir, trecs = R.split_frame(tf)
    _, ldir, _ = R.split_frame(lf)
    rec_lens = [8 * len(side) + len(data) for side, data in trecs]
    types = [typ for typ, _ in tdir]
    # all three record types, most blocks RAW (so that the frame passes 2^32 with the source)
    assert set(types) == {R.RAW, R.RLE, R.FSE}, types
    assert types.count(R.RAW) >= t - 3 and types[RLE_AT] == R.RLE, types
    n_total = k * len(tile) + len(tail)
    nb = k * t + 1
    out = {"header": R.header(nstates, R.kernel_class(0), block_size, ckpt, n_total),
           "tile_dir": tf[32: 32 + 4 * t], "tail_dir": lf[32: 36], "tile_rec": tf[32 + 4 * t:], "tail_rec": lf[36:],
           "rec_lens": rec_lens, "types": types, "tail_type": ldir[0][0], "n_total": n_total, "n_blocks": nb,
           "records_off": 32 + 4 * nb, "tile_blocks": t, "k": k}
    assert sum(rec_lens) == len(out["tile_rec"])
    out["frame_len"] = out["records_off"] + k * len(out["tile_rec"]) + len(out["tail_rec"])
    return out


def tiles_for(tile, tail, block_size, configs, least=1 << 32):
    """The smallest k for which the reference frame of every (ckpt, nstates)
    of `configs` is at least `least` + two tiles' records long."""
    k = 0
    for ckpt, nstates in configs:
        one = tiled_layout(tile, 1, tail, block_size, ckpt, nstates)
        per, t = len(one["tile_rec"]), one["tile_blocks"]
        fixed = 32 + 4 + len(one["tail_rec"])
        need = least + 2 * per - fixed
        k = max(k, -(-need // (per + 4 * t)))
    for ckpt, nstates in configs:
        lay = tiled_layout(tile, k, tail, block_size, ckpt, nstates)
        assert lay["frame_len"] >= least + 2 * len(lay["tile_rec"])
    return k


def tiled_frame(tile, k, tail, block_size, ckpt, nstates, device="cpu", layout=None):
    """The expected frame of tiled_source(tile, k, tail) as a uint8 tensor on `device`."""
    lay = layout or tiled_layout(tile, k, tail, block_size, ckpt, nstates)
    assert nstates in (1, 2) and lay["k"] == k
    u8 = lambda b: _tensor(np.frombuffer(b, dtype=np.uint8), device)  # noqa: E731
    t = lay["tile_blocks"]
    out = torch.empty(lay["frame_len"], dtype=torch.uint8, device=device)
    out[:32] = u8(lay["header"])
    at = 32
    _fill_repeats(out[at: at + 4 * t * k], u8(lay["tile_dir"]), k)
    at += 4 * t * k
    out[at: at + 4] = u8(lay["tail_dir"])
    at += 4
    assert at == lay["records_off"]
    per = len(lay["tile_rec"])
    _fill_repeats(out[at: at + per * k], u8(lay["tile_rec"]), k)
    at += per * k
    out[at:] = u8(lay["tail_rec"])
    assert at + len(lay["tail_rec"]) == lay["frame_len"]
    return out


def block_of_frame_offset(layout, frame_off):
    """(block, record start, record end): the block of the tiled frame whose
    record holds frame byte `frame_off`, from the reference directory's
    prefix sum."""
    per = len(layout["tile_rec"])
    rel = frame_off - layout["records_off"]
    assert 0 <= rel < per * layout["k"]
    tile_no, within = divmod(rel, per)
    start = 0
    for i, ln in enumerate(layout["rec_lens"]):
        if within < start + ln:
            lo = layout["records_off"] + tile_no * per + start
            return tile_no * layout["tile_blocks"] + i, lo, lo + ln
        start += ln
    raise AssertionError("offset past the tile's records")


def record_span(layout, block):
    """(start, end) of a tile block's record in the tiled frame: block_of_frame_offset's inverse."""
    tile_no, i = divmod(block, layout["tile_blocks"])
    assert 0 <= tile_no < layout["k"]
    lo = layout["records_off"] + tile_no * len(layout["tile_rec"]) + sum(layout["rec_lens"][:i])
    return lo, lo + layout["rec_lens"][i]


# ---------------------------------------------------------------- CRC-32
def _crc_join(a, b):
    """(crc, length) of A || B from those of A and of B."""
    return CR.combine(a[0], b[0], b[1]), a[1] + b[1]


def tiled_crc32(tile, k, tail):
    """zlib.crc32(tile * k + tail) by repeated squaring over k: no pass over the whole content."""
    tile, tail = bytes(tile), bytes(tail)
    acc, sq = (0, 0), (zlib.crc32(tile), len(tile))
    n = k
    while n:
        if n & 1:
            acc = _crc_join(acc, sq)  # the parts are all the same tile, so their order does not matter
        sq = _crc_join(sq, sq)
        n >>= 1
    assert acc[1] == k * len(tile)
    return _crc_join(acc, (zlib.crc32(tail), len(tail)))[0] if tail else acc[0]


def tiled_crc(tile, k, tail, check_log=16):
    """The reference check record (check_ref.record's bytes) of the tiled content."""
    B = 1 << check_log
    assert len(tile) % B == 0  # the tile's check blocks repeat with it
    crcs = CR.block_crcs(tile, check_log) * k + CR.block_crcs(tail, check_log)
    n = k * len(tile) + len(tail)
    assert len(crcs) == CR.n_cb_of(n, check_log)
    return CR.header(check_log, n, len(crcs), tiled_crc32(tile, k, tail)) + np.asarray(crcs, dtype="<u4").tobytes()


# ---------------------------------------------------------------- the estimate
def tiled_estimate(tile, k, tail, block_size, ckpt, nstates):
    """estimate_ref.frame_estimate of the tiled content: the predictions of
    the tile's blocks, k times, and the tail's."""
    te = E.block_estimates(E.counts_of(tile, block_size), len(tile), block_size, nstates=nstates, ckpt=ckpt)
    le = E.block_estimates(E.counts_of(tail, block_size), len(tail), block_size, nstates=nstates, ckpt=ckpt)
    assert len(le) == 1
    return 32 + 4 * (k * len(te) + 1) + k * sum(e[1] for e in te) + le[0][1]


# ---------------------------------------------------------------- the element images, as tensor ops
INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def _ints(x):
    """A contiguous 1-D tensor of 2-, 4- or 8-byte elements as the signed integers of its bit patterns."""
    w = x.element_size()
    assert w in INT and x.dim() == 1 and x.is_contiguous()
    return x.view(INT[w]), w


def _zigzag(d, w):
    """(d << 1) ^ (d >> (8 w - 1)), the shift arithmetic: 0 or -1, as the references' 0 - (d >>> (8 w - 1))."""
    z = d << 1
    z ^= d >> (8 * w - 1)
    return z


def planes_image(x):
    """planes_ref.image of a tensor's bytes: image[p * stride + i] = byte p of element i, pads zero."""
    x, w = _ints(x)
    n = x.numel()
    out = torch.zeros((w, PR.stride_of(n)), dtype=torch.uint8, device=x.device)
    if n:
        out[:, :n] = x.view(torch.uint8).view(n, w).t()
    return out.view(-1)


def planes_unimage(img, n_elems, dtype):
    """planes_ref.unimage as a tensor of `dtype`."""
    w = torch.empty(0, dtype=dtype).element_size()
    assert img.numel() == w * PR.stride_of(n_elems)
    if n_elems == 0:
        return torch.empty(0, dtype=dtype, device=img.device)
    return img.view(w, PR.stride_of(n_elems))[:, :n_elems].t().contiguous().view(-1).view(dtype)


def delta_image(x, restart=DR.RESTART):
    """delta_ref.image: zigzag of the wrapping differences of neighbours, the
    first element of every `restart` kept as it is, then byte planes."""
    x, w = _ints(x)
    d = x.clone()
    d[1:] -= x[:-1]
    d[::restart] = x[::restart]
    return planes_image(_zigzag(d, w))


def diff_image(x, base):
    """diff_ref.image: zigzag of the wrapping bit-pattern differences against `base`, then byte planes."""
    x, w = _ints(x)
    b, wb = _ints(base)
    assert w == wb and x.numel() == b.numel()
    return planes_image(_zigzag(x - b, w))
