"""tests/large_ref.py against the numpy references it restates, at sizes the
CPU oracle walks whole: the tiled frame against frame_ref.build_frame of the
tiled source, the tiled check record against check_ref.record and zlib, the
tiled estimate against estimate_ref, and the torch images against
planes_ref / delta_ref / diff_ref.  What tests/test_gpu_large.py compares the
library with past 4 GiB is pinned here."""
import zlib

import numpy as np
import pytest
import torch

import check_ref as CR
import delta_ref as DR
import diff_ref as FR
import estimate_ref as E
import frame_ref as R
import large_ref as L
import planes_ref as PR

BS, K, TAIL = 512, 3, 313


@pytest.fixture(scope="module")
def small():
    tile, tail = L.tile_and_tail(7, BS, TAIL)
    return tile, tail, np.concatenate([tile] * K + [tail])


def test_tile_requirements(small):
    tile, tail, raw = small
    assert len(tile) == L.TILE_BLOCKS * BS and len(tail) == TAIL
    assert np.array_equal(L.tiled_source(tile, K, tail).numpy(), raw)
    # the product's numbers: a wrap by 2^32 or 2^31 moves to another block of the tile
    assert (1 << 32) // L.BLOCK % L.TILE_BLOCKS == 1 and (1 << 31) // L.BLOCK % L.TILE_BLOCKS == 8
    for t in (16, 32):  # a tile that divides the wraps hides them: refused
        with pytest.raises(AssertionError, match="hides"):
            L.tile_and_tail(7, L.BLOCK, L.TAIL, tile_blocks=t)
        with pytest.raises(AssertionError, match="hides"):
            L.check_tile_blocks(t, L.BLOCK)
    rot = L.rotated(tile, BS)
    assert np.array_equal(rot[BS:], tile[:-BS]) and np.array_equal(rot[:BS], tile[-BS:])


@pytest.mark.parametrize("nstates,ckpt", [(2, 64), (2, 0), (1, 64)])
def test_tiled_frame_is_the_frame_of_the_tiled_source(small, nstates, ckpt):
    tile, tail, raw = small
    want = R.build_frame(raw, BS, ckpt, nstates)
    lay = L.tiled_layout(tile, K, tail, BS, ckpt, nstates)
    got = L.tiled_frame(tile, K, tail, BS, ckpt, nstates, layout=lay)
    assert got.dtype == torch.uint8 and got.numpy().tobytes() == want
    assert lay["frame_len"] == len(want) and lay["n_total"] == len(raw) and lay["n_blocks"] == K * L.TILE_BLOCKS + 1
    info, directory, records = R.split_frame(want)
    assert info["records_off"] == lay["records_off"]
    assert [t for t, _ in directory] == lay["types"] * K + [lay["tail_type"]]
    # the prefix sum: every record's first and last byte find their block
    pos = lay["records_off"]
    for b, (side, data) in enumerate(records[:-1]):
        ln = 8 * len(side) + len(data)
        assert L.block_of_frame_offset(lay, pos) == (b, pos, pos + ln)
        assert L.block_of_frame_offset(lay, pos + ln - 1) == (b, pos, pos + ln)
        assert L.record_span(lay, b) == (pos, pos + ln)
        pos += ln


def test_tiles_for_is_the_smallest(small):
    tile, tail, _ = small
    configs = [(64, 2), (0, 2), (64, 1)]
    least = 40000
    k = L.tiles_for(tile, tail, BS, configs, least)
    lens = lambda kk: [(len(R.build_frame(np.concatenate([tile] * kk + [tail]), BS, c, s)),  # noqa: E731
                        len(L.tiled_layout(tile, 1, tail, BS, c, s)["tile_rec"])) for c, s in configs]
    assert all(ln >= least + 2 * per for ln, per in lens(k))
    assert not all(ln >= least + 2 * per for ln, per in lens(k - 1))


def test_substituted_record_is_unequal(small):
    """The mutation the tile size exists for: block b + W's record in block
    b's place, W a wrap's block count, differs from the reference."""
    tile, tail, _ = small
    k = 40
    lay = L.tiled_layout(tile, k, tail, BS, 64, 2)
    ref = L.tiled_frame(tile, k, tail, BS, 64, 2, layout=lay)
    per = len(lay["tile_rec"])
    starts = np.concatenate([[0], np.cumsum(lay["rec_lens"])])
    for wrap in L.WRAPS:
        shift = (wrap // L.BLOCK) % L.TILE_BLOCKS  # what a wrap at 64 KiB blocks moves a block by in the tile
        for i in range(L.TILE_BLOCKS):
            j = (i + shift) % L.TILE_BLOCKS
            a = lay["tile_rec"][starts[i]: starts[i + 1]]
            b = lay["tile_rec"][starts[j]: starts[j + 1]]
            assert a != b, (wrap, i, j)
            if len(a) == len(b):  # the same length: substitute in place, the frame stays well formed
                bad = ref.clone()
                at = lay["records_off"] + 5 * per + int(starts[i])
                bad[at: at + len(a)] = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy())
                assert not torch.equal(bad, ref), (wrap, i, j)


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 8, 13])
def test_tiled_crc(k):
    tile, tail = L.tile_and_tail(11, 1024, 777)
    content = bytes(tile) * k + bytes(tail)
    assert L.tiled_crc32(tile, k, tail) == zlib.crc32(content)
    assert L.tiled_crc32(tile, k, tail[:-1]) == zlib.crc32(content[:-1])
    assert L.tiled_crc32(tile, k, b"") == zlib.crc32(bytes(tile) * k)
    for log in (8, 10):
        assert L.tiled_crc(tile, k, tail, log) == CR.record(content, log)


@pytest.mark.parametrize("nstates,ckpt", [(2, 64), (1, 0)])
def test_tiled_estimate(small, nstates, ckpt):
    tile, tail, raw = small
    want = E.frame_estimate(E.counts_of(raw, BS), len(raw), BS, nstates=nstates, ckpt=ckpt)
    assert L.tiled_estimate(tile, K, tail, BS, ckpt, nstates) == want


def patterns(w, n):
    """name -> n unsigned w-byte integers: random bit patterns, and the
    extremes next to each other so that every subtraction wraps."""
    rng = np.random.default_rng(0x1A26E + 16 * w + n)
    u = DR.UINT[w]
    top = (1 << (8 * w)) - 1
    rnd = np.frombuffer(rng.integers(0, 256, n * w, dtype=np.uint8).tobytes(), dtype=u)
    ext = np.asarray([0, top, 1 << (8 * w - 1), (1 << (8 * w - 1)) - 1, 1, top - 1], dtype=np.uint64).astype(u)
    return {"random": rnd, "extremes": ext[rng.integers(0, len(ext), n)],
            "cycle": ext[np.arange(n) % len(ext)]}


def as_tensor(a, w):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.dtype(f"<i{w}")).copy())


@pytest.mark.parametrize("n", [70001, 4097, 4096, 1, 0])
@pytest.mark.parametrize("w", [2, 4, 8])
def test_torch_images_against_numpy(w, n):
    pats = patterns(w, n)
    for name, a in pats.items():
        raw = PR.raw_bytes(a)
        x = as_tensor(a, w)
        assert x.numel() == n and x.element_size() == w
        got = L.planes_image(x)
        assert got.numpy().tobytes() == PR.image(raw, w).tobytes(), (name, "planes")
        back = L.planes_unimage(got, n, L.INT[w])
        assert back.dtype == L.INT[w] and PR.raw_bytes(back.numpy()).tobytes() == raw.tobytes(), (name, "unimage")
        assert PR.raw_bytes(back.numpy()).tobytes() == PR.unimage(PR.image(raw, w), w, n).tobytes()
        assert L.delta_image(x).numpy().tobytes() == DR.image(raw, w).tobytes(), (name, "delta")
        for bname, b in pats.items():
            want = FR.image(raw, PR.raw_bytes(b), w)
            assert L.diff_image(x, as_tensor(b, w)).numpy().tobytes() == want.tobytes(), (name, bname, "diff")
        # float dtypes of the width go by their bit patterns
        fl = {2: torch.bfloat16, 4: torch.float32, 8: torch.float64}[w]
        assert torch.equal(L.planes_image(x.view(fl)), got)
