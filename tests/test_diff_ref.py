"""The diff frame's numpy restatement (tests/diff_ref.py), no GPU: it
round-trips at every width and at the sizes round a 16-element group;
identical tensors code to run-length blocks alone; and on the tensors the
format is for the reference-built diff frame is at most half of the
reference-built plane frame (DESIGN.md section 5 "Diff" has the table:
measured 0.12 to 0.42 there, 0.55 and 0.66 on the two rows bounded by 0.75,
1.05 on the control bounded by 1.08).  The library does not run here except
as a check that it exports the calls at all."""
import numpy as np
import pytest

import diff_ref as DF
import frame_ref as R

SIZES = [0, 1, 15, 16, 17, 4097]


def test_the_library_has_the_diff_calls():
    from entropy_coders_amd import BlockCodec, _lib, diff_compress, diff_decompress  # noqa: F401

    assert hasattr(_lib.load(), "fsehip_diff_compress") and hasattr(BlockCodec, "compress_diff")
    assert _lib.SEALED_KINDS[3] == "diff" and _lib.KIND_DIFF == 4


@pytest.mark.parametrize("op", ["sub", "xor"])
@pytest.mark.parametrize("w", DF.WIDTHS)
def test_image_round_trips(w, op):
    rng = np.random.default_rng(0xD1FF + w)
    for n in SIZES:
        raw = rng.integers(0, 256, n * w, dtype=np.uint8)  # full-range bits: the difference wraps both ways
        base = rng.integers(0, 256, n * w, dtype=np.uint8)
        img = DF.image(raw, base, w, op)
        assert img.size == w * DF.stride_of(n)
        assert DF.unimage(img, base, w, n, op).tobytes() == raw.tobytes(), (w, n)
        assert not img.reshape(w, -1)[:, n:].any(), "pads are zero"


def test_image_by_hand():
    """uint16 against a base: +3, -2, the wrap 0 - 0x8000 and 0x8000 - 1."""
    x = np.array([5, 3, 0, 0x8000, 7], dtype=np.uint16)
    b = np.array([2, 5, 0x8000, 1, 7], dtype=np.uint16)
    z = DF.zigzag(x, b, 2)
    assert z.tolist() == [6, 3, 0xFFFF, 0xFFFE, 0]  # d = 0x8000 -> 0xFFFF; d = 0x7FFF -> 0xFFFE
    img = DF.image(DF.raw_bytes(x), DF.raw_bytes(b), 2)
    assert img.size == 32 and img[0] == 6 and img[16 + 2] == 0xFF and not img[5:16].any()
    assert DF.zigzag(x, b, 2, op="xor").tolist() == [7, 6, 0x8000, 0x8001, 0]


@pytest.mark.parametrize("w", DF.WIDTHS)
def test_frames_round_trip(w):
    rng = np.random.default_rng(0xF4A3E + w)
    for n in SIZES:
        b = rng.integers(0, 1 << 8 * min(w, 7), n).astype(DF.UINT[w])
        a = (b + rng.integers(-3, 40, n).astype(DF.UINT[w])).astype(DF.UINT[w])
        buf = DF.build(a, b, 4096, 128, 2)
        assert buf[:4] == b"FSEB" and len(buf) <= DF.bound(n, w, 4096)
        got = DF.decode(buf, b)
        assert got[:2] == (w, n) and got[2].tobytes() == a.tobytes()
    assert len(DF.build(np.zeros(0, DF.UINT[w]), np.zeros(0, DF.UINT[w]), 65536, 128, 2)) == 48


@pytest.mark.parametrize("w", DF.WIDTHS)
@pytest.mark.parametrize("n,block", [(1, 4096), (4097, 4096), (70000, 65536)])
def test_identical_tensors_are_run_length_blocks_alone(w, n, block):
    a = np.random.default_rng(n + w).integers(0, 256, n * w, dtype=np.uint8).view(DF.UINT[w])
    buf = DF.build(a, a.copy(), block, 128, 2)
    n_blocks = R.n_blocks_of(w * DF.stride_of(n), block)
    assert len(buf) == 16 + 32 + 5 * n_blocks  # per block 4 directory bytes and the one repeated byte
    assert DF.decode(buf, a)[2].tobytes() == a.tobytes()


def test_another_base_decodes_to_other_bytes():
    """The container does not identify its base: whatever base is given, the decode succeeds."""
    a = np.arange(100, dtype=np.uint32)
    buf = DF.build(a + 7, a, 4096, 128, 2)
    assert DF.decode(buf, a)[2].view(np.uint32).tolist() == (a + 7).tolist()
    assert DF.decode(buf, a + 1)[2].view(np.uint32).tolist() == (a + 8).tolist()


@pytest.fixture(scope="module")
def rows():
    return DF.table_rows()


def sizes(rows, name):
    x, b = rows[name]
    diff, plain = len(DF.build(x, b, 65536, 64, 2)), DF.plain_size(x)
    print(f"\n[diff] {name}: diff frame {diff / x.nbytes:.3f}, plain {plain / x.nbytes:.3f} of the raw bytes, "
          f"ratio {diff / plain:.3f}")
    return diff, plain


@pytest.mark.parametrize("name", DF.TARGETS)
def test_size_condition_on_the_target_tensors(rows, name):
    diff, plain = sizes(rows, name)
    assert diff <= 0.5 * plain


@pytest.mark.parametrize("name", DF.GAINS)
def test_size_condition_on_the_rows_that_gain_less(rows, name):
    diff, plain = sizes(rows, name)
    assert diff <= 0.75 * plain


def test_the_control_stays_close_to_the_plane_frame(rows):
    diff, plain = sizes(rows, DF.CONTROL)
    assert diff <= 1.08 * plain
    x, _ = rows[DF.CONTROL]
    assert diff <= DF.bound(x.size, 2, 65536)
