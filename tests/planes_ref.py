"""The plane frame (include/fsehip.h section 2d) restated in numpy over
tests/frame_ref.py: a helper for the plane tests, not a test.

  image        raw elements -> plane image (reshape(-1, w).T into zero-padded strides)
  unimage      plane image -> raw bytes
  header       the 16 header bytes
  build        elements -> plane frame, the inner frame from frame_ref.build_frame
  decode       plane frame -> raw bytes, through frame_ref.decode_frame

Nothing here calls the library under test.
"""
import struct

import numpy as np

import frame_ref as R

MAGIC = b"FSEP"


def stride_of(n_elems):
    return (n_elems + 15) // 16 * 16


def raw_bytes(a):
    """The bytes of an array (any dtype) as a flat uint8 array."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def image(raw, w):
    """image[k * stride + i] = raw[i * w + k], pads zero."""
    raw = np.asarray(raw, dtype=np.uint8)
    assert raw.size % w == 0
    n = raw.size // w
    out = np.zeros((w, stride_of(n)), dtype=np.uint8)
    out[:, :n] = raw.reshape(-1, w).T
    return out.reshape(-1)


def unimage(img, w, n_elems):
    img = np.asarray(img, dtype=np.uint8)
    return np.ascontiguousarray(img.reshape(w, stride_of(n_elems))[:, :n_elems].T).reshape(-1)


def header(w, n_elems, version=1, reserved=0, magic=MAGIC):
    return magic + struct.pack("<BBHQ", version, w, reserved, n_elems)


def bound(n_elems, w, block_size):
    return 16 + R.bound(w * stride_of(n_elems), block_size)


def build(elems, block_size, ckpt, nstates, table_log=0, sidecars=None):
    """The plane frame of an array of 2-, 4- or 8-byte items."""
    a = np.ascontiguousarray(elems).reshape(-1)
    w = a.dtype.itemsize
    img = image(raw_bytes(a), w)
    return header(w, a.size) + R.build_frame(img, block_size, ckpt, nstates, table_log, sidecars=sidecars)


def decode(buf):
    """(w, n_elems, raw bytes) of a plane frame."""
    buf = bytes(buf)
    assert buf[:4] == MAGIC and len(buf) >= 48
    version, w, reserved, n = struct.unpack("<BBHQ", buf[4:16])
    assert version == 1 and w in (2, 4, 8) and reserved == 0
    img = np.frombuffer(R.decode_frame(buf[16:]), dtype=np.uint8)
    assert img.size == w * stride_of(n)
    return w, n, unimage(img, w, n)
