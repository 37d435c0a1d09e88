"""The diff frame (include/fsehip.h section 2h) restated in numpy over
tests/planes_ref.py and tests/frame_ref.py: a helper for the diff tests, not
a test.

  image        raw element bytes of x and of the base -> diff image (subtract, zigzag, byte planes)
  unimage      diff image and the base's raw bytes -> raw element bytes of x
  header       the 16 header bytes
  build        elements and base -> diff frame, the inner frame from frame_ref.build_frame
  decode       diff frame and the base -> raw bytes, through frame_ref.decode_frame
  table_rows   the tensors of the size table in DESIGN.md section 5 "Diff"

op="xor" (image, unimage, build) is the variant the DESIGN table compares; the
format itself has none.  Nothing here calls the library under test.
"""
import struct

import numpy as np

import frame_ref as R
import planes_ref as PR

MAGIC = b"FSEB"
WIDTHS = (1, 2, 4, 8)
UINT = {1: np.uint8, 2: np.dtype("<u2"), 4: np.dtype("<u4"), 8: np.dtype("<u8")}

stride_of = PR.stride_of
raw_bytes = PR.raw_bytes


def zigzag(x, b, w, op="sub"):
    """z_i of the unsigned w-byte integers x against b (arithmetic mod 2^(8 w))."""
    x, b = np.asarray(x, dtype=UINT[w]), np.asarray(b, dtype=UINT[w])
    assert x.shape == b.shape
    if op == "xor":
        return x ^ b
    d = x - b
    return (d << 1) ^ (np.zeros_like(d) - (d >> (8 * w - 1)))


def unzigzag(z, b, w, op="sub"):
    z, b = np.asarray(z, dtype=UINT[w]), np.asarray(b, dtype=UINT[w])
    if op == "xor":
        return z ^ b
    return b + ((z >> 1) ^ (np.zeros_like(z) - (z & 1)))


def _planes(z, w):
    z = raw_bytes(z)
    if w > 1:
        return PR.image(z, w)
    out = np.zeros(stride_of(z.size), dtype=np.uint8)
    out[:z.size] = z
    return out


def image(raw, base_raw, w, op="sub"):
    """image[k * stride + i] = byte k of z_i, pads zero."""
    raw = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8))
    base_raw = np.ascontiguousarray(np.asarray(base_raw, dtype=np.uint8))
    assert raw.size % w == 0 and raw.size == base_raw.size
    return _planes(zigzag(raw.view(UINT[w]), base_raw.view(UINT[w]), w, op), w)


def unimage(img, base_raw, w, n_elems, op="sub"):
    img = np.asarray(img, dtype=np.uint8)
    base_raw = np.ascontiguousarray(np.asarray(base_raw, dtype=np.uint8))
    assert base_raw.size == n_elems * w
    z = PR.unimage(img, w, n_elems) if w > 1 else img[:n_elems]
    return raw_bytes(unzigzag(np.ascontiguousarray(z).view(UINT[w]), base_raw.view(UINT[w]), w, op))


def header(w, n_elems, version=1, reserved=0, magic=MAGIC):
    return magic + struct.pack("<BBHQ", version, w, reserved, n_elems)


def bound(n_elems, w, block_size):
    return 16 + R.bound(w * stride_of(n_elems), block_size)


def build(elems, base, block_size, ckpt, nstates, table_log=0, sidecars=None, op="sub"):
    """The diff frame of an array of 1-, 2-, 4- or 8-byte items against a
    base of the same item size and count."""
    a, b = np.ascontiguousarray(elems).reshape(-1), np.ascontiguousarray(base).reshape(-1)
    w = a.dtype.itemsize
    assert b.dtype.itemsize == w and a.size == b.size
    img = image(raw_bytes(a), raw_bytes(b), w, op)
    return header(w, a.size) + R.build_frame(img, block_size, ckpt, nstates, table_log, sidecars=sidecars)


def decode(buf, base, op="sub"):
    """(w, n_elems, raw bytes) of a diff frame against the base array."""
    buf = bytes(buf)
    assert buf[:4] == MAGIC and len(buf) >= 48
    version, w, reserved, n = struct.unpack("<BBHQ", buf[4:16])
    assert version == 1 and w in WIDTHS and reserved == 0
    img = np.frombuffer(R.decode_frame(buf[16:]), dtype=np.uint8)
    assert img.size == w * stride_of(n)
    return w, n, unimage(img, raw_bytes(base), w, n, op)


def _bits(t):
    """A torch tensor's bit patterns as a numpy integer array of its width."""
    import torch

    view = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(view).numpy().copy()


def table_rows(n=1 << 18, seed=1):
    """The tensors of the size table in DESIGN.md section 5 "Diff": name ->
    (x, base), numpy integer arrays of the bit patterns.  The float rows are
    drawn in table order from one torch generator: the fp32 master w32 =
    randn(n) * 0.02 first, then each row's noise (the Adam row: m, then g;
    the control: its second tensor); the int32 table from numpy's generators
    3 (the table), 4 (which rows change) and 5 (their new values)."""
    import torch

    g = torch.Generator().manual_seed(seed)
    randn = lambda: torch.randn(n, generator=g)  # noqa: E731
    w32 = randn() * 0.02
    rows = {}
    rows["bf16 master 1e-4"] = (_bits((w32 + 1e-4 * randn()).bfloat16()), _bits(w32.bfloat16()))
    rows["bf16 master 1e-5"] = (_bits((w32 + 1e-5 * randn()).bfloat16()), _bits(w32.bfloat16()))
    rows["bf16 fine-tune 2e-3"] = (_bits((w32 + 2e-3 * randn()).bfloat16()), _bits(w32.bfloat16()))
    rows["fp16 master 1e-4"] = (_bits((w32 + 1e-4 * randn()).half()), _bits(w32.half()))
    rows["fp32 master 1e-5"] = (_bits(w32 + 1e-5 * randn()), _bits(w32))
    rows["fp32 master 1e-4"] = (_bits(w32 + 1e-4 * randn()), _bits(w32))
    m = randn() * 1e-3
    grad = randn() * 1e-3
    rows["fp32 Adam m"] = (_bits(0.9 * m + 0.1 * grad), _bits(m))
    q8 = lambda w: torch.clamp(torch.round(w / 0.02 * 32), -128, 127).to(torch.int8)  # noqa: E731
    rows["int8 weights 1e-4"] = (_bits(q8(w32 + 1e-4 * randn())), _bits(q8(w32)))
    table = np.random.default_rng(3).integers(0, 1 << 20, n).astype(np.int32)
    newer = table.copy()
    pick = np.random.default_rng(4).choice(n, n // 50, replace=False)
    newer[pick] = np.random.default_rng(5).integers(0, 1 << 20, pick.size).astype(np.int32)
    rows["int32 table 2% replaced"] = (newer, table)
    rows["bf16 unrelated (control)"] = (_bits((randn() * 0.02).bfloat16()), _bits(w32.bfloat16()))
    return rows


# the rows the format is for: at most HALF of the plane frame (the byte frame at w = 1)
TARGETS = ("bf16 master 1e-4", "bf16 master 1e-5", "int8 weights 1e-4", "int32 table 2% replaced")
# rows that gain, less: at most THREE_QUARTERS
GAINS = ("fp16 master 1e-4", "fp32 master 1e-5")
CONTROL = "bf16 unrelated (control)"


def plain_size(a, block_size=65536, ckpt=64, nstates=2):
    """What the diff frame is compared with: the plane frame of `a`, at item
    size 1 the byte frame of its 16-padded bytes."""
    a = np.ascontiguousarray(a).reshape(-1)
    if a.dtype.itemsize > 1:
        return len(PR.build(a, block_size, ckpt, nstates))
    raw = np.zeros(stride_of(a.size), dtype=np.uint8)
    raw[:a.size] = raw_bytes(a)
    return len(R.build_frame(raw, block_size, ckpt, nstates))
