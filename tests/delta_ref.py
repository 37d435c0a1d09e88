"""The delta frame (include/fsehip.h section 2e) restated in numpy over
tests/planes_ref.py and tests/frame_ref.py: a helper for the delta tests, not
a test.

  image        raw element bytes -> delta image (delta with restarts, zigzag, byte planes)
  unimage      delta image -> raw element bytes
  header       the 16 header bytes
  build        elements -> delta frame, the inner frame from frame_ref.build_frame
  decode       delta frame -> raw bytes, through frame_ref.decode_frame

Nothing here calls the library under test.
"""
import struct

import numpy as np

import frame_ref as R
import planes_ref as PR

MAGIC = b"FSED"
RESTART = 4096
WIDTHS = (1, 2, 4, 8)
UINT = {1: np.uint8, 2: np.dtype("<u2"), 4: np.dtype("<u4"), 8: np.dtype("<u8")}

stride_of = PR.stride_of
raw_bytes = PR.raw_bytes


def zigzag(x, w, restart=RESTART, zz=True):
    """z_i of the unsigned w-byte integers x (arithmetic mod 2^(8 w))."""
    x = np.asarray(x, dtype=UINT[w])
    d = x.copy()
    d[1:] -= x[:-1]
    d[::restart] = x[::restart]
    if not zz:
        return d
    return (d << 1) ^ (np.zeros_like(d) - (d >> (8 * w - 1)))


def unzigzag(z, w, restart=RESTART):
    z = np.asarray(z, dtype=UINT[w])
    d = (z >> 1) ^ (np.zeros_like(z) - (z & 1))
    n = d.size
    padded = np.zeros((n + restart - 1) // restart * restart, dtype=UINT[w])
    padded[:n] = d
    return np.cumsum(padded.reshape(-1, restart), axis=1, dtype=UINT[w]).reshape(-1)[:n]


def image(raw, w, restart=RESTART, zz=True):
    """image[k * stride + i] = byte k of z_i, pads zero."""
    raw = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8))
    assert raw.size % w == 0
    z = raw_bytes(zigzag(raw.view(UINT[w]), w, restart, zz))
    if w > 1:
        return PR.image(z, w)
    out = np.zeros(stride_of(z.size), dtype=np.uint8)
    out[:z.size] = z
    return out


def unimage(img, w, n_elems):
    img = np.asarray(img, dtype=np.uint8)
    z = PR.unimage(img, w, n_elems) if w > 1 else img[:n_elems]
    return raw_bytes(unzigzag(np.ascontiguousarray(z).view(UINT[w]), w))


def header(w, n_elems, version=1, reserved=0, magic=MAGIC):
    return magic + struct.pack("<BBHQ", version, w, reserved, n_elems)


def bound(n_elems, w, block_size):
    return 16 + R.bound(w * stride_of(n_elems), block_size)


def build(elems, block_size, ckpt, nstates, table_log=0, sidecars=None, restart=RESTART, zz=True):
    """The delta frame of an array of 1-, 2-, 4- or 8-byte items (restart and
    zz other than the format's: the variants DESIGN.md compares)."""
    a = np.ascontiguousarray(elems).reshape(-1)
    w = a.dtype.itemsize
    img = image(raw_bytes(a), w, restart, zz)
    return header(w, a.size) + R.build_frame(img, block_size, ckpt, nstates, table_log, sidecars=sidecars)


def decode(buf):
    """(w, n_elems, raw bytes) of a delta frame."""
    buf = bytes(buf)
    assert buf[:4] == MAGIC and len(buf) >= 48
    version, w, reserved, n = struct.unpack("<BBHQ", buf[4:16])
    assert version == 1 and w in WIDTHS and reserved == 0
    img = np.frombuffer(R.decode_frame(buf[16:]), dtype=np.uint8)
    assert img.size == w * stride_of(n)
    return w, n, unimage(img, w, n)


def table_rows(n=1 << 18, seed=1):
    """The tensors of the size table in DESIGN.md section 5 "Delta", drawn in
    this order from one generator: name -> array."""
    rng = np.random.default_rng(seed)
    rows = {}
    rows["int64 sorted ids"] = np.cumsum(rng.geometric(1 / 1000, n)).astype(np.int64)
    rows["int32 CSR offsets"] = np.cumsum(rng.poisson(40, n)).astype(np.int32)
    rows["int16 sensor walk"] = np.cumsum(rng.integers(-20, 21, n)).astype(np.int16)
    rows["int32 clustered ids"] = (np.repeat(rng.integers(0, 1 << 30, n // 64), 64)
                                   + rng.integers(-500, 500, n)).astype(np.int32)
    rows["int32 uniform"] = rng.integers(0, 1 << 31, n).astype(np.int32)
    return rows


TARGETS = ("int64 sorted ids", "int32 CSR offsets", "int16 sensor walk", "int32 clustered ids")
