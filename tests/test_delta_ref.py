"""The delta frame's numpy restatement (tests/delta_ref.py), no GPU: it
round-trips at every width and at the sizes round a restart, and on the tensors
the format is for the reference-built delta frame is at most 0.6 of the
reference-built plane frame (DESIGN.md section 5 "Delta" has the table; measured
0.29 to 0.52).  The library does not run here except as a check that it
exports the calls at all."""
import numpy as np
import pytest

import delta_ref as DR
import planes_ref as PR

SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5]


def test_the_library_has_the_delta_calls():
    from entropy_coders_amd import BlockCodec, _lib, delta_compress, delta_decompress  # noqa: F401

    assert _lib.DELTA_RESTART == DR.RESTART
    assert hasattr(_lib.load(), "fsehip_delta_compress") and hasattr(BlockCodec, "compress_delta")


@pytest.mark.parametrize("w", DR.WIDTHS)
def test_image_round_trips(w):
    rng = np.random.default_rng(0xDE17A + w)
    for n in SIZES:
        raw = rng.integers(0, 256, n * w, dtype=np.uint8)  # full-range bits: wraparound both ways
        img = DR.image(raw, w)
        assert img.size == w * DR.stride_of(n)
        assert DR.unimage(img, w, n).tobytes() == raw.tobytes(), (w, n)
        planes = img.reshape(w, -1)
        assert not planes[:, n:].any(), "pads are zero"


def test_image_by_hand():
    """int16 0, 3, 1, -32768 (as 0x8000: the delta wraps), then a restart."""
    x = np.zeros(4100, dtype=np.int16)
    x[:4] = [0, 3, 1, -32768]
    x[4095:4098] = [7, 7, 5]
    z = DR.zigzag(x.view(np.uint16), 2)
    # deltas 0, 3, -2, 0x8000 - 1 = 0x7FFF, (0 - 0x8000) = 0x8000 -> zigzag 0xFFFF
    assert z[:5].tolist() == [0, 6, 3, 0xFFFE, 0xFFFF]
    assert z[4095:4098].tolist() == [14, 14, 3]  # 7 from 0; the restart stores 7 itself; -2
    img = DR.image(PR.raw_bytes(x), 2)
    assert img[1] == 6 and img[DR.stride_of(4100) + 3] == 0xFF


@pytest.mark.parametrize("w", DR.WIDTHS)
def test_frames_round_trip(w):
    rng = np.random.default_rng(0xF4A3E + w)
    for n in (0, 1, 4097, 3 * 4096 + 5):
        a = np.cumsum(rng.integers(-3, 40, n)).astype(DR.UINT[w])
        buf = DR.build(a, 4096, 128, 2)
        assert len(buf) <= DR.bound(n, w, 4096)
        assert DR.decode(buf)[2].tobytes() == a.tobytes()
    assert len(DR.build(np.zeros(0, DR.UINT[w]), 65536, 128, 2)) == 48


@pytest.fixture(scope="module")
def rows():
    return DR.table_rows()


@pytest.mark.parametrize("name", DR.TARGETS)
def test_size_condition_on_the_target_tensors(rows, name):
    a = rows[name]
    delta = len(DR.build(a, 65536, 64, 2))
    planes = len(PR.build(a, 65536, 64, 2))
    print(f"\n[delta] {name}: delta frame {delta / a.nbytes:.3f}, plane frame {planes / a.nbytes:.3f} of the raw bytes, "
          f"ratio {delta / planes:.3f}")
    assert delta <= 0.6 * planes


def test_uniform_random_stays_within_the_bound(rows):
    a = rows["int32 uniform"]
    assert len(DR.build(a, 65536, 64, 2)) <= DR.bound(a.size, 4, 65536)
