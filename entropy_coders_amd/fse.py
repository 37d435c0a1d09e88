"""Python mirror of the reference crate's API for this path (tests, bench).

Reference-shaped calls (host bytes in, bytes out; lib.rs:146-248,
histogram.rs:18-66) and a batched device codec over torch tensors.  All
compute goes through libfsehip.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from ._lib import (EST_NONE, KIND_DIFF, KIND_PACK, KIND_SEALED, KIND_SPACK, KIND_VPACK, KINDS, MCHECK_BASES, SEALED_KINDS,
                   BitStackReaderState, McheckInfo,
                   BitStackWriterState, BitStreamReaderState, CheckInfo, DecodeTable, DeltaInfo, DiffInfo, EncodeTable,
                   FrameInfo, FrameParams, FrameRange, FseError, Histogram, NormHistogram, PackInfo, PackMember, Params,
                   PlanesInfo, PlanesRange, check, load)


def _buf(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class PackHead:
    """What BlockCodec.pack_info reads from a pack frame (fsehip.h section
    2j) or a versioned pack (section 2k): `container` says which, "pack" or
    "vpack"; only the latter's `kinds` may hold "diff"."""

    def __init__(self, info, members, inner, container="pack"):
        self.info, self.members, self.inner, self.container = info, members, inner, container
        n = info.n_members
        self.kinds = [_PACK_KIND_NAMES[members[m].kind] for m in range(n)]
        self.elem_bytes = [int(members[m].elem_bytes) for m in range(n)]
        self.n_elems = [int(members[m].n_elems) for m in range(n)]


_PACK_KIND_NAMES = {1: "planes", 2: "delta", KIND_DIFF: "diff"}


class _ElemKind:
    """What tells the element frames (fsehip.h sections 2d, 2e, 2h) apart:
    the C names' prefix and their names of the two bare transforms, the
    element widths taken, the info class, the label used in messages and
    whether the calls take a base tensor (after the source or destination
    pointer)."""

    def __init__(self, prefix: str, split: str, merge: str, widths: tuple, info, label: str, based: bool = False):
        self.prefix, self.split, self.merge = prefix, split, merge
        self.widths, self.info, self.label, self.based = widths, info, label, based
        self.takes = ", ".join(map(str, widths[:-1])) + f" or {widths[-1]}"  # "2, 4 or 8"


_ELEM = {"planes": _ElemKind("fsehip_planes_", "split", "merge", (2, 4, 8), PlanesInfo, "plane"),
         "delta": _ElemKind("fsehip_delta_", "encode", "decode", (1, 2, 4, 8), DeltaInfo, "delta"),
         "diff": _ElemKind("fsehip_diff_", "encode", "decode", (1, 2, 4, 8), DiffInfo, "diff", based=True)}

# fsehip_estimate_base's five entries by FSEHIP_KIND_*: entry 3 (sealed) is no choice of container
_BASE_KINDS = KINDS + (None, "diff")

_tls = threading.local()


def _out(cap: int) -> np.ndarray:
    """A per-thread output buffer of >= cap bytes, reused across calls (the
    calls return copies): allocating a fresh 16 MiB array per call costs
    more than a small decode."""
    b = getattr(_tls, "out", None)
    if b is None or len(b) < cap:
        b = np.empty(max(cap, 1), dtype=np.uint8)
        _tls.out = b
    return b


def compress2(src) -> tuple[bytes, int]:
    """`fse_compress2(src, &mut dst) -> usize` (lib.rs:146): (bytes, payload bits)."""
    a = _buf(src)
    lib = load()
    cap = int(lib.fsehip_slot_bytes(max(len(a), 16), 12))
    dst = _out(cap)
    n = C.c_size_t(0)
    bits = C.c_uint64(0)
    check(lib.fse_compress2(_p(a), len(a), _p(dst), cap, C.byref(n), C.byref(bits)), "fse_compress2")
    return dst[: n.value].tobytes(), bits.value


def compress2_log(src, table_log: int) -> tuple[bytes, int]:
    """`Histogram::new(src).normalize(L)` + fse_compress2 body (histogram.rs:95)."""
    a = _buf(src)
    lib = load()
    cap = int(lib.fsehip_slot_bytes(max(len(a), 16), 12))
    dst = _out(cap)
    n = C.c_size_t(0)
    bits = C.c_uint64(0)
    check(lib.fse_compress2_log(_p(a), len(a), table_log, _p(dst), cap, C.byref(n), C.byref(bits)),
          "fse_compress2_log")
    return dst[: n.value].tobytes(), bits.value


def decompress2(src, cap: int = 1 << 24) -> bytes:
    """`fse_decompress2(src, &mut dst) -> Option<usize>` (lib.rs:215)."""
    a = _buf(src)
    lib = load()
    dst = _out(cap)
    n = C.c_size_t(0)
    check(lib.fse_decompress2(_p(a), len(a), _p(dst), cap, C.byref(n)), "fse_decompress2")
    return dst[: n.value].tobytes()


def compress(src) -> tuple[bytes, int]:
    """`fse_compress(src, &mut dst) -> (NormHistogram, usize)` (lib.rs:112): the
    1-state format; (bytes, payload bits).  The header in the bytes is the
    returned NormHistogram."""
    a = _buf(src)
    lib = load()
    cap = int(lib.fsehip_slot_bytes(max(len(a), 16), 12))
    dst = _out(cap)
    n = C.c_size_t(0)
    bits = C.c_uint64(0)
    check(lib.fse_compress(_p(a), len(a), _p(dst), cap, C.byref(n), C.byref(bits)), "fse_compress")
    return dst[: n.value].tobytes(), bits.value


def decompress(src, cap: int = 1 << 24) -> bytes:
    """`fse_decompress(src, &mut dst) -> Option<usize>` (lib.rs:187)."""
    a = _buf(src)
    lib = load()
    dst = _out(cap)
    n = C.c_size_t(0)
    check(lib.fse_decompress(_p(a), len(a), _p(dst), cap, C.byref(n)), "fse_decompress")
    return dst[: n.value].tobytes()


def decompress2_many(streams, dst_stride: int, nstates: int = 2, raw: bool = False, dst=None):
    """`fse_decompress2_many` / `fse_decompress_many` (nstates 1): many crate
    streams from host memory in one call, each decoded as `fse_decompress2`
    (lib.rs:215) would within dst_stride bytes.  Returns a list with, per
    stream, its bytes or the name of its status; with raw=True the call's own
    outputs instead: (dst, lengths, statuses) as numpy arrays (dst may be
    passed in, n * dst_stride bytes, to reuse one buffer across calls)."""
    from ._lib import STATUS

    if nstates not in (1, 2):
        raise ValueError(f"nstates must be 1 or 2, not {nstates!r}")
    lib = load()
    bufs = [_buf(x) for x in streams]
    n = len(bufs)
    ptrs = np.array([b.ctypes.data if len(b) else 0 for b in bufs] or [0], dtype=np.uintp)
    lens = np.array([len(b) for b in bufs] or [0], dtype=np.uintp)
    if dst is None:
        dst = np.empty(max(n, 1) * dst_stride, dtype=np.uint8)
    elif not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous
              and dst.flags.writeable and dst.nbytes >= n * dst_stride):
        # the C call writes n * dst_stride bytes through the raw pointer
        raise ValueError(f"dst must be a writeable C-contiguous uint8 ndarray of >= {n * dst_stride} bytes")
    out_lens = np.zeros(max(n, 1), dtype=np.uintp)
    st = np.zeros(max(n, 1), dtype=np.int32)
    fn = lib.fse_decompress2_many if nstates == 2 else lib.fse_decompress_many
    check(fn(_p(ptrs), _p(lens), n, _p(dst), dst_stride, _p(out_lens), _p(st)), "fse_decompress2_many")
    if raw:
        return dst, out_lens[:n], st[:n]
    return [dst[i * dst_stride: i * dst_stride + int(out_lens[i])].tobytes() if st[i] == 0 else
            STATUS.get(int(st[i]), str(int(st[i]))) for i in range(n)]


def decompress_streams(streams, out_stride: int, nstates: int = 2, max_table_log: int = 11, device=None):
    """`fsehip_decompress_streams`: many crate streams (no sidecar, no raw
    length) decoded at once on the GPU, each as `fse_decompress2` (nstates 2)
    or `fse_decompress` (1) would, within out_stride bytes.  Returns a list
    with, per stream, its bytes or the name of its status."""
    import torch

    from ._lib import STATUS

    dev = torch.device(device or "cuda")
    stride = max(512, (max((len(x) for x in streams), default=1) + 255) // 256 * 256)
    host = np.zeros(len(streams) * stride, dtype=np.uint8)
    for i, x in enumerate(streams):
        host[i * stride: i * stride + len(x)] = np.frombuffer(bytes(x), dtype=np.uint8)
    d_in = torch.from_numpy(host).to(dev)
    lens = torch.tensor([len(x) for x in streams], dtype=torch.int32, device=dev)
    out = torch.empty(len(streams) * out_stride, dtype=torch.uint8, device=dev)
    out_len = torch.zeros(len(streams), dtype=torch.int32, device=dev)
    status = torch.zeros(len(streams), dtype=torch.int32, device=dev)
    check(load().fsehip_decompress_streams(nstates, max_table_log, C.c_void_p(d_in.data_ptr()), stride,
                                           C.c_void_p(lens.data_ptr()), len(streams), C.c_void_p(out.data_ptr()),
                                           out_stride, C.c_void_p(out_len.data_ptr()),
                                           C.c_void_p(status.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
          "fsehip_decompress_streams")
    torch.cuda.synchronize(dev)
    host_out, ol, st = out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
    return [host_out[i * out_stride: i * out_stride + int(ol[i])].tobytes() if st[i] == 0 else
            STATUS.get(int(st[i]), str(int(st[i]))) for i in range(len(streams))]


def compress2_many(buffers, nstates: int = 2, dst_stride=None, raw: bool = False, dst=None):
    """`fse_compress2_many` / `fse_compress_many` (nstates 1): many host
    buffers of any lengths in one call, each compressed as `fse_compress2`
    (lib.rs:146) would into an empty buffer of dst_stride bytes (default: a
    capacity that holds the longest).  Returns a list with, per buffer,
    (bytes, payload bits) or the name of its status; with raw=True the call's
    own outputs instead: (dst, lengths, payload bits, statuses) as numpy
    arrays (dst may be passed in, n * dst_stride bytes).  An entry of
    `buffers` may be (None, n): a null pointer of length n."""
    from ._lib import STATUS

    if nstates not in (1, 2):
        raise ValueError(f"nstates must be 1 or 2, not {nstates!r}")
    lib = load()
    null = [isinstance(x, tuple) and x[0] is None for x in buffers]
    bufs = [np.empty(0, dtype=np.uint8) if z else _buf(x) for x, z in zip(buffers, null)]
    n = len(bufs)
    ptrs = np.array([b.ctypes.data if len(b) else 0 for b in bufs] or [0], dtype=np.uintp)
    lens = np.array([int(x[1]) if z else len(b) for x, b, z in zip(buffers, bufs, null)] or [0], dtype=np.uintp)
    if dst_stride is None:
        dst_stride = int(lib.fsehip_stream_out_bytes(int(lens.max()) if n else 0, 11))
    if dst is None:
        dst = np.zeros(max(n, 1) * dst_stride, dtype=np.uint8)
    elif not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous
              and dst.flags.writeable and dst.nbytes >= n * dst_stride):
        raise ValueError(f"dst must be a writeable C-contiguous uint8 ndarray of >= {n * dst_stride} bytes")
    out_lens = np.zeros(max(n, 1), dtype=np.uintp)
    bits = np.zeros(max(n, 1), dtype=np.uint64)
    st = np.zeros(max(n, 1), dtype=np.int32)
    fn = lib.fse_compress2_many if nstates == 2 else lib.fse_compress_many
    check(fn(_p(ptrs), _p(lens), n, _p(dst), dst_stride, _p(out_lens), _p(bits), _p(st)), "fse_compress2_many")
    if raw:
        return dst, out_lens[:n], bits[:n], st[:n]
    return [(dst[i * dst_stride: i * dst_stride + int(out_lens[i])].tobytes(), int(bits[i])) if st[i] == 0 else
            STATUS.get(int(st[i]), str(int(st[i]))) for i in range(n)]


def compress_streams(buffers, nstates: int = 2, table_log: int = 0, device=None, out_caps=None, max_table_log: int = 0,
                     raw: bool = False):
    """`fsehip_compress_streams`: many inputs of any lengths compressed at once
    on the GPU, each as `fse_compress2` (nstates 2) / `fse_compress` (1) would
    -- with table_log as `fse_compress2_log`.  The inputs are laid out back to
    back at 16-byte aligned offsets; each output region has out_caps[i] bytes
    (default `fsehip_stream_out_bytes`) and the regions are 64 bytes apart,
    the gaps filled with 0xA5.  Returns a list with, per stream, (bytes,
    payload bits) or the name of its status; with raw=True (statuses, lengths,
    payload bits, out bytes as numpy, descriptors) for bounds checks."""
    import torch

    from ._lib import STATUS, StreamDesc

    lib = load()
    dev = torch.device(device or "cuda")
    bufs = [_buf(x) for x in buffers]
    n = len(bufs)
    lmax = max_table_log or (max(11, min(table_log, 15)) if table_log else 11)
    caps = [int(lib.fsehip_stream_out_bytes(len(b), lmax)) for b in bufs] if out_caps is None else list(out_caps)
    desc = (StreamDesc * max(n, 1))()
    so = oo = 0
    for i, b in enumerate(bufs):
        desc[i] = StreamDesc(so, oo, len(b), caps[i])
        so += (len(b) + 15) // 16 * 16
        oo += (caps[i] + 15) // 16 * 16 + 64
    host = np.zeros(max(so, 16), dtype=np.uint8)
    for i, b in enumerate(bufs):
        host[desc[i].src_off: desc[i].src_off + len(b)] = b
    d_src = torch.from_numpy(host).to(dev)
    d_desc = torch.from_numpy(np.frombuffer(bytes(desc), dtype=np.uint8).copy()).to(dev)
    out = torch.full((max(oo, 16),), 0xA5, dtype=torch.uint8, device=dev)
    comp_len = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    bits = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    check(lib.fsehip_compress_streams(nstates, table_log, max_table_log, C.c_void_p(d_src.data_ptr()),
                                      C.c_void_p(d_desc.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(comp_len.data_ptr()), C.c_void_p(bits.data_ptr()),
                                      C.c_void_p(status.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
          "fsehip_compress_streams")
    torch.cuda.synchronize(dev)
    ho, cl, pb, st = out.cpu().numpy(), comp_len.cpu().numpy()[:n], bits.cpu().numpy()[:n], status.cpu().numpy()[:n]
    if raw:
        return st, cl, pb, ho, [(d.src_off, d.out_off, d.src_len, d.out_cap) for d in desc[:n]]
    return [(ho[desc[i].out_off: desc[i].out_off + int(cl[i])].tobytes(), int(pb[i]) & 0xFFFFFFFF) if st[i] == 0 else
            STATUS.get(int(st[i]), str(int(st[i]))) for i in range(n)]


def histogram_count(src) -> tuple[np.ndarray, int]:
    """`Histogram::new(data)` (histogram.rs:18-66): (counts[256], table_len)."""
    a = _buf(src)
    lib = load()
    counts = np.zeros(256, dtype=np.uint32)
    tl = C.c_uint32(0)
    check(lib.histogram_count(_p(a), len(a), _p(counts), C.byref(tl)), "histogram_count")
    return counts, tl.value


# ---------------------------------------------------------------- building blocks
def histogram_new(src) -> Histogram:
    """`Histogram::new(data)` (histogram.rs:18-66)."""
    a = _buf(src)
    h = Histogram()
    check(load().histogram_new(_p(a), len(a), C.byref(h)), "histogram_new")
    return h


def normalize(h: Histogram, log2: int) -> NormHistogram:
    """`Histogram::normalize(log2)` (histogram.rs:95-155)."""
    nh = NormHistogram()
    check(load().histogram_normalize(C.byref(h), log2, C.byref(nh)), "histogram_normalize")
    return nh


def normalize_optimal(h: Histogram) -> NormHistogram:
    """`Histogram::normalize_optimal` (histogram.rs:281-284)."""
    nh = NormHistogram()
    check(load().histogram_normalize_optimal(C.byref(h), C.byref(nh)), "histogram_normalize_optimal")
    return nh


def norm_histogram_new(src) -> NormHistogram:
    """`NormHistogram::new(data)` (histogram.rs:299-303)."""
    a = _buf(src)
    nh = NormHistogram()
    check(load().norm_histogram_new(_p(a), len(a), C.byref(nh)), "norm_histogram_new")
    return nh


def norm_histogram_write(nh: NormHistogram) -> tuple[bytes, int]:
    """`NormHistogram::write(&mut Vec)` (histogram.rs:376-431): (bytes, bits written)."""
    dst = np.zeros(1024, dtype=np.uint8)
    n = C.c_size_t(0)
    bits = C.c_uint64(0)
    check(load().norm_histogram_write(C.byref(nh), _p(dst), len(dst), C.byref(n), C.byref(bits)),
          "norm_histogram_write")
    return dst[: n.value].tobytes(), bits.value


def norm_histogram_read(data) -> tuple[NormHistogram, int]:
    """`NormHistogram::read(slice)` (histogram.rs:436-505): (histogram, bytes consumed)."""
    a = _buf(data)
    nh = NormHistogram()
    used = C.c_size_t(0)
    check(load().norm_histogram_read(_p(a), len(a), C.byref(nh), C.byref(used)), "norm_histogram_read")
    return nh, used.value


def encode_table_new(nh: NormHistogram) -> EncodeTable:
    """`EncodeTable::new(&hist)` (fse.rs:88-189) as plain data."""
    t = EncodeTable()
    check(load().encode_table_new(C.byref(nh), C.byref(t)), "encode_table_new")
    return t


def decode_table_new(nh: NormHistogram) -> DecodeTable:
    """`DecodeTable::new(&hist)` (fse.rs:269-338) as plain data."""
    t = DecodeTable()
    check(load().decode_table_new(C.byref(nh), C.byref(t)), "decode_table_new")
    return t


def compress_nh(src) -> tuple[bytes, int, NormHistogram]:
    """`fse_compress(src, &mut dst) -> (NormHistogram, usize)` (lib.rs:112) with
    the histogram returned: (bytes, payload bits, NormHistogram)."""
    a = _buf(src)
    lib = load()
    cap = int(lib.fsehip_slot_bytes(max(len(a), 16), 12))
    dst = _out(cap)
    n = C.c_size_t(0)
    bits = C.c_uint64(0)
    nh = NormHistogram()
    check(lib.fse_compress_nh(_p(a), len(a), _p(dst), cap, C.byref(n), C.byref(bits), C.byref(nh)), "fse_compress_nh")
    return dst[: n.value].tobytes(), bits.value, nh


# ---------------------------------------------------------------- bitstream
def bitstack_write(vals, widths, prefix: bytes = b"") -> tuple[bytes, int]:
    """BitStackWriter::new(&mut vec) over a vec holding `prefix`, then
    write_bits_unmasked per field + finish (writer.rs:14-222): (the vec's
    bytes, bits written)."""
    v = np.ascontiguousarray(vals, dtype=np.uint32)
    w = np.ascontiguousarray(widths, dtype=np.uint8)
    cap = len(prefix) + len(v) * 4 + 16
    dst = np.zeros(cap, dtype=np.uint8)
    dst[: len(prefix)] = np.frombuffer(bytes(prefix), dtype=np.uint8)
    n = C.c_size_t(len(prefix))
    bits = C.c_uint64(0)
    check(load().bitstack_write(_p(v), _p(w), len(v), _p(dst), cap, C.byref(n), C.byref(bits)), "bitstack_write")
    return dst[: n.value].tobytes(), bits.value


def bitstack_read(data, widths) -> tuple[list, int, bool]:
    """BitStackReader::new + read(width) per field, top down (stack_reader.rs):
    (values read, number of successful reads, finish())."""
    a = _buf(data)
    w = np.ascontiguousarray(widths, dtype=np.uint8)
    out = np.zeros(max(len(w), 1), dtype=np.uint32)
    nr = C.c_size_t(0)
    fin = C.c_int(0)
    check(load().bitstack_read(_p(a), len(a), _p(w), len(w), _p(out), C.byref(nr), C.byref(fin)), "bitstack_read")
    return [int(x) for x in out[: nr.value]], nr.value, bool(fin.value)


EOF_STATUS = -18  # FSE_ERR_EOF: the reference's None / Err(UnexpectedEof)


class BitStackReader:
    """BitStackReader (stack_reader.rs:5-227) over the C-ABI cursor
    (fsehip.h section 1c): one O(1) call per method.  `peek` / `read` /
    `read_no_reload` return None where the crate returns None."""

    def __init__(self, data):
        self._buf = _buf(data)  # the cursor points into this buffer
        self.state = BitStackReaderState()
        self._lib = load()
        check(self._lib.bitstack_reader_new(C.byref(self.state), _p(self._buf), len(self._buf)),
              "BitStackReader::new")

    def _val(self, fn, nbits):
        v = C.c_uint32(0)
        rc = fn(C.byref(self.state), nbits, C.byref(v))
        if rc == EOF_STATUS:
            return None
        check(rc, fn.__name__)
        return v.value

    def peek(self, nbits: int):
        return self._val(self._lib.bitstack_reader_peek, nbits)

    def read(self, nbits: int):
        return self._val(self._lib.bitstack_reader_read, nbits)

    def read_no_reload(self, nbits: int):
        return self._val(self._lib.bitstack_reader_read_no_reload, nbits)

    def advance_no_reload(self, nbits: int) -> None:
        check(self._lib.bitstack_reader_advance_no_reload(C.byref(self.state), nbits), "advance_no_reload")

    def reload(self) -> None:
        check(self._lib.bitstack_reader_reload(C.byref(self.state)), "reload")

    def available(self) -> int:
        return int(self._lib.bitstack_reader_available(C.byref(self.state)))

    def finish(self) -> bool:
        return bool(self._lib.bitstack_reader_finish(C.byref(self.state)))


class BitStreamReader:
    """BitStreamReader (stream_reader.rs:5-136) over the C-ABI cursor.
    `peek` / `read` / `advance_by` raise EOFError where the crate returns
    Err(UnexpectedEof)."""

    def __init__(self, data, total_bits: int):
        self._buf = _buf(data)
        self.state = BitStreamReaderState()
        self._lib = load()
        check(self._lib.bitstream_reader_new(C.byref(self.state), _p(self._buf), len(self._buf), total_bits),
              "BitStreamReader::new")

    def _rc(self, rc: int, what: str) -> None:
        if rc == EOF_STATUS:
            raise EOFError(what)
        check(rc, what)

    def peek(self, nbits: int) -> int:
        v = C.c_uint32(0)
        self._rc(self._lib.bitstream_reader_peek(C.byref(self.state), nbits, C.byref(v)), "peek")
        return v.value

    def read(self, nbits: int) -> int:
        v = C.c_uint32(0)
        self._rc(self._lib.bitstream_reader_read(C.byref(self.state), nbits, C.byref(v)), "read")
        return v.value

    def advance_by(self, nbits: int) -> None:
        self._rc(self._lib.bitstream_reader_advance_by(C.byref(self.state), nbits), "advance_by")

    def available(self) -> int:
        return int(self._lib.bitstream_reader_available(C.byref(self.state)))

    def finish(self) -> tuple[bytes, int, int]:
        b, rem, off = C.c_size_t(0), C.c_uint64(0), C.c_uint32(0)
        check(self._lib.bitstream_reader_finish(C.byref(self.state), C.byref(b), C.byref(rem), C.byref(off)), "finish")
        return self._buf[b.value:].tobytes(), rem.value, off.value

    def finish_byte(self) -> bytes:
        return self._buf[int(self._lib.bitstream_reader_finish_byte(C.byref(self.state))):].tobytes()


class BitStackWriter:
    """BitStackWriter (writer.rs:5-223) appending to a buffer that holds
    `prefix`, over the C-ABI cursor; `finish()` returns (the buffer's bytes,
    bits written)."""

    def __init__(self, prefix: bytes = b"", cap: int = 1 << 16):
        self._dst = np.zeros(len(prefix) + cap, dtype=np.uint8)
        self._dst[: len(prefix)] = np.frombuffer(bytes(prefix), dtype=np.uint8)
        self.state = BitStackWriterState()
        self._lib = load()
        check(self._lib.bitstack_writer_new(C.byref(self.state), _p(self._dst), len(self._dst), len(prefix)),
              "BitStackWriter::new")

    def write_bits(self, val: int, nbits: int) -> None:
        check(self._lib.bitstack_writer_write_bits(C.byref(self.state), val, nbits), "write_bits")

    def write_bits_unmasked(self, val: int, nbits: int) -> None:
        check(self._lib.bitstack_writer_write_bits_unmasked(C.byref(self.state), val, nbits), "write_bits_unmasked")

    def write_bits_raw(self, val: int, nbits: int) -> None:
        check(self._lib.bitstack_writer_write_bits_raw(C.byref(self.state), val, nbits), "write_bits_raw")

    def write_bits_raw_unmasked(self, val: int, nbits: int) -> None:
        check(self._lib.bitstack_writer_write_bits_raw_unmasked(C.byref(self.state), val, nbits),
              "write_bits_raw_unmasked")

    def flush(self) -> None:
        check(self._lib.bitstack_writer_flush(C.byref(self.state)), "flush")

    def finish(self) -> tuple[bytes, int]:
        n, bits = C.c_size_t(0), C.c_uint64(0)
        check(self._lib.bitstack_writer_finish(C.byref(self.state), C.byref(n), C.byref(bits)), "finish")
        return self._dst[: n.value].tobytes(), bits.value


BITS_READ, BITS_PEEK, BITS_ADVANCE = 0, 1, 2  # FSE_BITS_* (include/fsehip.h)


def bitstream_read(data, total_bits: int, widths, ops=None) -> tuple[list, int, int]:
    """BitStreamReader::new(slice, total_bits) and one call per field
    (stream_reader.rs:56-119): read(width), or with `ops` peek(width)
    (BITS_PEEK) / advance_by(width) (BITS_ADVANCE, value 0).  Returns (values
    of the steps that returned Ok, their number, available() after them)."""
    a = _buf(data)
    w = np.ascontiguousarray(widths, dtype=np.uint8)
    out = np.zeros(max(len(w), 1), dtype=np.uint32)
    nr = C.c_size_t(0)
    left = C.c_uint64(0)
    if ops is None:
        check(load().bitstream_read(_p(a), len(a), total_bits, _p(w), len(w), _p(out), C.byref(nr), C.byref(left)),
              "bitstream_read")
    else:
        o = np.ascontiguousarray(ops, dtype=np.uint8)
        if len(o) != len(w):
            raise ValueError("one op per field")
        check(load().bitstream_read_ops(_p(a), len(a), total_bits, _p(w), _p(o), len(w), _p(out), C.byref(nr),
                                        C.byref(left)), "bitstream_read_ops")
    return [int(x) for x in out[: nr.value]], nr.value, left.value


class BlockCodec:
    """Batched device codec: 64 KiB blocks (configurable) over torch tensors.

    compress(src) -> CompressedBlocks (slots, lengths, sidecar, status), all
    resident on the device; decompress(cb) -> uint8 tensor.  Work is queued
    on torch's current stream.
    """

    def __init__(self, block_size: int = 65536, table_log: int = 0, ckpt_interval: int = 128,
                 device=None, nstates: int = 2):
        import torch

        self.torch = torch
        self.device = torch.device(device or "cuda")
        self.block_size = block_size
        self.table_log = table_log
        self.ckpt_interval = ckpt_interval
        self.nstates = nstates  # 2: fse_compress2 blocks (lib.rs:146), 1: fse_compress (lib.rs:112)
        self.max_table_log = max(11, table_log) if table_log else 11
        self.lib = load()
        self.slot_bytes = int(self.lib.fsehip_slot_bytes(block_size, self.max_table_log))
        self.side_per_block = int(self.lib.fsehip_sidecar_per_block_ns(block_size, ckpt_interval, nstates))

    def params(self) -> Params:
        return Params(self.block_size, self.table_log, self.ckpt_interval, self.max_table_log, self.nstates)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def release_workspace(self) -> None:
        """`fsehip_release_workspace` for this codec's device and torch's
        current stream: frees the decode workspace (decode tables, and the
        deferred-symbol states: 2 bytes per output byte of the last
        sidecar-less batch) after the queued work."""
        check(self.lib.fsehip_release_workspace(self.device.index if self.device.index is not None else
                                                self.torch.cuda.current_device(), self._stream()),
              "fsehip_release_workspace")

    def rank_fallbacks(self, reset: bool = False) -> dict:
        """`fsehip_rank_fallbacks` on this codec's device: tables whose atomic
        ranks failed their self-check and were rebuilt with peer-mask ranks
        (batch encoder, decode-table builds, building-block table calls)."""
        import ctypes as C

        out = (C.c_uint32 * 3)()
        dev = self.device.index if self.device.index is not None else self.torch.cuda.current_device()
        check(self.lib.fsehip_rank_fallbacks(dev, C.byref(out), 1 if reset else 0), "fsehip_rank_fallbacks")
        return {"encode": int(out[0]), "decode_tables": int(out[1]), "table_calls": int(out[2])}

    def n_blocks(self, n_total: int) -> int:
        return (n_total + self.block_size - 1) // self.block_size

    def alloc(self, n_total: int) -> dict:
        t = self.torch
        nb = self.n_blocks(n_total)
        return {
            "n_total": n_total,
            "out": t.empty(nb * self.slot_bytes, dtype=t.uint8, device=self.device),
            "comp_len": t.zeros(nb, dtype=t.int32, device=self.device),
            "payload_bits": t.zeros(nb, dtype=t.int32, device=self.device),
            "sidecar": t.zeros(max(nb * self.side_per_block, 1), dtype=t.int64, device=self.device),
            "status": t.zeros(nb, dtype=t.int32, device=self.device),
        }

    def compress_into(self, src, cb: dict) -> None:
        p = self.params()
        rc = self.lib.fsehip_compress_blocks(
            C.byref(p), C.c_void_p(src.data_ptr()), cb["n_total"], C.c_void_p(cb["out"].data_ptr()),
            self.slot_bytes, C.c_void_p(cb["comp_len"].data_ptr()),
            C.c_void_p(cb["payload_bits"].data_ptr()),
            C.c_void_p(cb["sidecar"].data_ptr()) if self.ckpt_interval else None,
            C.c_void_p(cb["status"].data_ptr()), self._stream())
        check(rc, "fsehip_compress_blocks")

    def compress(self, src) -> dict:
        cb = self.alloc(src.numel())
        self.compress_into(src, cb)
        return cb

    def decompress_into(self, cb: dict, out, status, use_sidecar: bool = True) -> None:
        p = self.params()
        side = C.c_void_p(cb["sidecar"].data_ptr()) if (use_sidecar and self.ckpt_interval) else None
        rc = self.lib.fsehip_decompress_blocks(
            C.byref(p), C.c_void_p(cb["out"].data_ptr()), self.slot_bytes,
            C.c_void_p(cb["comp_len"].data_ptr()), side, C.c_void_p(out.data_ptr()), cb["n_total"],
            C.c_void_p(status.data_ptr()), self._stream())
        check(rc, "fsehip_decompress_blocks")

    def decompress(self, cb: dict, use_sidecar: bool = True):
        t = self.torch
        out = t.empty(cb["n_total"], dtype=t.uint8, device=self.device)
        status = t.zeros(self.n_blocks(cb["n_total"]), dtype=t.int32, device=self.device)
        self.decompress_into(cb, out, status, use_sidecar)
        return out, status

    def build_sidecar(self, cb: dict):
        """`fsehip_build_sidecar`: decode blocks that carry no sidecar (e.g.
        from the CPU crate) and record their sidecar.  Returns (out, sidecar,
        status) device tensors."""
        t = self.torch
        nb = self.n_blocks(cb["n_total"])
        out = t.empty(cb["n_total"], dtype=t.uint8, device=self.device)
        side = t.zeros(max(nb * self.side_per_block, 1), dtype=t.int64, device=self.device)
        status = t.zeros(nb, dtype=t.int32, device=self.device)
        p = self.params()
        check(self.lib.fsehip_build_sidecar(
            C.byref(p), C.c_void_p(cb["out"].data_ptr()), self.slot_bytes, C.c_void_p(cb["comp_len"].data_ptr()),
            C.c_void_p(out.data_ptr()), cb["n_total"], C.c_void_p(side.data_ptr()), C.c_void_p(status.data_ptr()),
            self._stream()), "fsehip_build_sidecar")
        return out, side, status

    def build_dtables(self, cb: dict) -> dict:
        """Decode tables for every block of `cb` (fsehip_build_dtables): the
        pre-built tables of decode-only workloads (C3)."""
        t = self.torch
        nb = self.n_blocks(cb["n_total"])
        per = int(self.lib.fsehip_dtable_bytes(self.max_table_log))
        tabs = {"dt": t.empty(nb * per // 4, dtype=t.int32, device=self.device),
                "info": t.empty(nb, dtype=t.int32, device=self.device)}
        self.build_dtables_into(cb, tabs)
        return tabs

    def build_dtables_into(self, cb: dict, tabs: dict) -> None:
        p = self.params()
        check(self.lib.fsehip_build_dtables(
            C.byref(p), C.c_void_p(cb["out"].data_ptr()), self.slot_bytes, C.c_void_p(cb["comp_len"].data_ptr()),
            self.n_blocks(cb["n_total"]), C.c_void_p(tabs["dt"].data_ptr()), C.c_void_p(tabs["info"].data_ptr()),
            self._stream()), "fsehip_build_dtables")

    def decompress_dt_into(self, cb: dict, tabs: dict, out, status, use_sidecar: bool = True) -> None:
        """Decode with pre-built tables (2-state needs the sidecar; 1-state
        without one runs the serial reference-order decoder)."""
        p = self.params()
        side = C.c_void_p(cb["sidecar"].data_ptr()) if (use_sidecar and self.ckpt_interval) else None
        check(self.lib.fsehip_decompress_blocks_dt(
            C.byref(p), C.c_void_p(cb["out"].data_ptr()), self.slot_bytes, C.c_void_p(cb["comp_len"].data_ptr()),
            side, C.c_void_p(tabs["dt"].data_ptr()),
            C.c_void_p(tabs["info"].data_ptr()), C.c_void_p(out.data_ptr()), cb["n_total"],
            C.c_void_p(status.data_ptr()), self._stream()), "fsehip_decompress_blocks_dt")

    def generate(self, kind: int, prob: float, seed: int, n_total: int):
        t = self.torch
        out = t.empty(n_total, dtype=t.uint8, device=self.device)
        check(self.lib.fsehip_generate(kind, prob, seed, self.block_size, C.c_void_p(out.data_ptr()),
                                       n_total, self._stream()), "fsehip_generate")
        return out

    # ------------------------------------------------------------ the frame
    # fsehip.h section 2b: one self-describing buffer for any input (RAW /
    # RLE fallback per block), this library's own container.
    def frame_bound(self, n: int) -> int:
        """`fsehip_frame_bound`: a capacity no frame of n bytes exceeds."""
        return int(self.lib.fsehip_frame_bound(n, self.block_size))

    def compress_frame_into(self, src, frame, frame_len, result, chunk_blocks: int = 0) -> None:
        """`fsehip_frame_compress`, no synchronisation: `frame` a uint8 device
        tensor of >= frame_bound(src.numel()) bytes (any alignment),
        `frame_len` one int64, `result` two int32 (frame status, blocks not
        stored as FSE)."""
        p = FrameParams(self.block_size, self.table_log, self.ckpt_interval, self.max_table_log, self.nstates,
                        chunk_blocks)
        check(self.lib.fsehip_frame_compress(
            C.byref(p), C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(frame.data_ptr()), frame.numel(),
            C.c_void_p(frame_len.data_ptr()), C.c_void_p(result.data_ptr()), self._stream()), "fsehip_frame_compress")

    def compress_frame(self, src, chunk_blocks: int = 0):
        """Compress any uint8 device tensor (empty included) into one frame: a
        uint8 device tensor of the frame's exact length.  One
        synchronisation, to read the length."""
        t = self.torch
        frame = t.empty(self.frame_bound(src.numel()), dtype=t.uint8, device=self.device)
        frame_len = t.zeros(1, dtype=t.int64, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self.compress_frame_into(src, frame, frame_len, result, chunk_blocks)
        return frame[: int(frame_len.item())]

    @staticmethod
    def frame_info(frame) -> FrameInfo:
        """`fsehip_frame_read_header` of a frame given as bytes, a numpy array
        or a tensor (its first 32 bytes come to the host); raises FseError
        (BAD_FRAME) for anything that is not a frame header."""
        if hasattr(frame, "data_ptr"):  # a torch tensor
            head = frame[:32].cpu().numpy().tobytes()
        else:
            head = bytes(memoryview(frame)[:32])
        a = np.frombuffer(head, dtype=np.uint8)
        info = FrameInfo()
        check(load().fsehip_frame_read_header(_p(a), len(a), C.byref(info)), "fsehip_frame_read_header")
        return info

    def decompress_frame_into(self, frame, info: FrameInfo, out, block_status, result, chunk_blocks: int = 0) -> None:
        """`fsehip_frame_decompress`, no synchronisation: `out` >= info.n_total
        bytes (16-byte aligned), `block_status` info.n_blocks int32 or None,
        `result` two int32 (frame status, failed blocks)."""
        check(self.lib.fsehip_frame_decompress(
            C.byref(info), chunk_blocks, C.c_void_p(frame.data_ptr()), frame.numel(), C.c_void_p(out.data_ptr()),
            out.numel(), C.c_void_p(block_status.data_ptr()) if block_status is not None else None,
            C.c_void_p(result.data_ptr()), self._stream()), "fsehip_frame_decompress")

    def decompress_frame(self, frame, chunk_blocks: int = 0):
        """Decode a frame (a uint8 device tensor) from its bytes alone: the
        codec's own parameters play no part.  Returns (out, block_status);
        raises FseError for a frame-level error (BAD_FRAME)."""
        t = self.torch
        info = self.frame_info(frame)
        out = t.empty(info.n_total, dtype=t.uint8, device=self.device)
        status = t.zeros(info.n_blocks, dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self.decompress_frame_into(frame, info, out, status, result, chunk_blocks)
        check(int(result[0].item()), "frame")
        return out, status

    @staticmethod
    def frame_ranges(ranges):
        """(src_off, len, dst_off) triples as the fsehip_frame_range array the
        C call reads."""
        arr = (FrameRange * max(len(ranges), 1))(*[FrameRange(int(s), int(ln), int(d)) for s, ln, d in ranges])
        arr.empty = len(ranges) == 0
        return arr

    def decompress_frame_ranges_into(self, frame, info: FrameInfo, ranges, out, range_status, result,
                                     chunk_blocks: int = 0) -> None:
        """`fsehip_frame_decompress_ranges`, no synchronisation: `ranges` a
        sequence of (src_off, len, dst_off), or what `frame_ranges` made of
        one (a caller that repeats a call builds the array once); range r's
        raw bytes go to out[dst_off: dst_off + len] (`out` a uint8 device
        tensor, any alignment).  `range_status` len(ranges) int32 or None,
        `result` two int32 (frame status, ranges with a failed block)."""
        arr = ranges if isinstance(ranges, C.Array) else self.frame_ranges(ranges)
        n = 0 if getattr(arr, "empty", False) else len(arr)
        check(self.lib.fsehip_frame_decompress_ranges(
            C.byref(info), chunk_blocks, C.c_void_p(frame.data_ptr()), frame.numel(), arr, n,
            C.c_void_p(out.data_ptr()), out.numel(),
            C.c_void_p(range_status.data_ptr()) if range_status is not None else None,
            C.c_void_p(result.data_ptr()), self._stream()), "fsehip_frame_decompress_ranges")

    def decompress_frame_ranges(self, frame, ranges, chunk_blocks: int = 0):
        """Decode the raw byte ranges [(src_off, len), ...] of a frame (a uint8
        device tensor) without decoding the rest.  The ranges are packed back
        to back into one uint8 tensor; returns (list of views of it, one per
        range, and the int32 range statuses).  Raises FseError for a
        frame-level error (BAD_FRAME)."""
        t = self.torch
        info = self.frame_info(frame)
        packed, at = [], 0
        for s, ln in ranges:
            packed.append((s, ln, at))
            at += ln
        out = t.empty(at, dtype=t.uint8, device=self.device)
        status = t.zeros(len(packed), dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self.decompress_frame_ranges_into(frame, info, packed, out, status, result, chunk_blocks)
        check(int(result[0].item()), "frame")
        return [out[d: d + ln] for _, ln, d in packed], status

    def decompress_frame_range(self, frame, offset: int, length: int, chunk_blocks: int = 0):
        """Raw bytes [offset, offset + length) of a frame as a uint8 device
        tensor; raises FseError for a frame-level error or with the status of
        the first failed block the range touches."""
        views, status = self.decompress_frame_ranges(frame, [(offset, length)], chunk_blocks)
        check(int(status[0].item()), "frame range")
        return views[0]

    # ------------------------------------------------------------ the element frames
    # fsehip.h sections 2d and 2e: one container under two names.  The plane
    # frame puts byte k of every element into plane k and codes the planes by
    # one frame.  The delta frame first takes the zigzag differences of
    # neighbouring elements, with a restart every 4,096: for integer tensors
    # that grow (sorted ids, offsets, timestamps); any dtype of 1, 2, 4 or 8
    # bytes round-trips, floats gain nothing.  The container stores the element
    # width; dtype and shape stay with the caller.  The diff frame (section 2h)
    # takes the zigzag differences against a base tensor of the same dtype and
    # element count that the receiver already holds, and needs that base to
    # decode; the container does not identify it (a sealed buffer's checksums
    # tell a wrong one).  The `_elem_*` methods take the kind, "planes",
    # "delta" or "diff" (a row of _ELEM), and `base` for "diff" alone; the
    # public names forward.
    def _elem_fn(self, kind: str, name: str):
        return getattr(self.lib, _ELEM[kind].prefix + name)

    def _elem_call(self, kind: str, name: str, *args) -> None:
        check(self._elem_fn(kind, name)(*args), _ELEM[kind].prefix + name)

    @staticmethod
    def _elem_width(kind: str, x) -> int:
        k, w = _ELEM[kind], x.element_size()
        if w == 1 and 1 not in k.widths:  # the plane frame
            raise ValueError(f"compress_{kind} is for 2-, 4- and 8-byte elements; 1-byte tensors go to compress_frame")
        if w not in k.widths:
            raise ValueError(f"element size {w}: the {k.label} frame takes {k.takes} bytes")
        if not x.is_contiguous():
            raise ValueError(f"compress_{kind} needs a contiguous tensor")
        return w

    def _elem_base(self, kind: str, base, n_elems: int, dtype) -> tuple:
        """The base argument of a call of the kind: () for a kind without one,
        else the base's pointer after these checks (ValueError): a contiguous
        device tensor of `dtype` and n_elems elements."""
        if not _ELEM[kind].based:
            if base is not None:
                raise ValueError(f"the {_ELEM[kind].label} frame takes no base")
            return ()
        if base is None:
            raise ValueError("the diff frame needs its base tensor")
        if not hasattr(base, "data_ptr") or not base.is_cuda:
            raise ValueError("base must be a device tensor")
        if not base.is_contiguous():
            raise ValueError("base must be contiguous")
        if base.dtype != dtype or base.numel() != n_elems:
            raise ValueError(f"base has {base.numel()} elements of {base.dtype}, the tensor {n_elems} of {dtype}")
        return (C.c_void_p(base.data_ptr()),)

    def _elem_out(self, out, n_elems: int, dtype):
        """The caller's `out` of a decode after its checks, or a fresh tensor."""
        if out is None:
            return self.torch.empty(n_elems, dtype=dtype, device=self.device)
        if not out.is_contiguous() or out.dtype != dtype or out.numel() != n_elems:
            raise ValueError(f"out must be a contiguous tensor of {n_elems} elements of {dtype}")
        return out

    def _elem_bound(self, kind: str, n_elems: int, elem_bytes: int) -> int:
        return int(self._elem_fn(kind, "bound")(n_elems, elem_bytes, self.block_size))

    def _elem_scratch_bytes(self, kind: str, n_elems: int, elem_bytes: int) -> int:
        return int(self._elem_fn(kind, "scratch_bytes")(n_elems, elem_bytes))

    def _elem_split(self, kind: str, x, base=None):
        """The image of a contiguous device tensor (uint8, pads zeroed)."""
        w = self._elem_width(kind, x)
        b = self._elem_base(kind, base, x.numel(), x.dtype)
        image = self.torch.empty(self._elem_scratch_bytes(kind, x.numel(), w), dtype=self.torch.uint8,
                                 device=self.device)
        self._elem_call(kind, _ELEM[kind].split, w, C.c_void_p(x.data_ptr()), *b, x.numel(),
                        C.c_void_p(image.data_ptr()), self._stream())
        return image

    def _elem_merge(self, kind: str, image, n_elems: int, dtype, base=None, out=None):
        """n_elems elements of `dtype` from an image (into `out` when given)."""
        b = self._elem_base(kind, base, n_elems, dtype)
        out = self._elem_out(out, n_elems, dtype)
        self._elem_call(kind, _ELEM[kind].merge, out.element_size(), C.c_void_p(image.data_ptr()), n_elems,
                        C.c_void_p(out.data_ptr()), *b, self._stream())
        return out

    def _elem_compress_into(self, kind: str, x, scratch, out, out_len, result, chunk_blocks: int = 0,
                            base=None) -> None:
        """The compress call, no synchronisation: `scratch` a uint8 device
        tensor of >= the kind's scratch_bytes, `out` of >= its bound bytes (any
        alignment), `out_len` one int64, `result` two int32."""
        w = self._elem_width(kind, x)
        b = self._elem_base(kind, base, x.numel(), x.dtype)
        p = self._frame_params(chunk_blocks)
        self._elem_call(kind, "compress", C.byref(p), w, C.c_void_p(x.data_ptr()), *b, x.numel(),
                        C.c_void_p(scratch.data_ptr()), scratch.numel(), C.c_void_p(out.data_ptr()), out.numel(),
                        C.c_void_p(out_len.data_ptr()), C.c_void_p(result.data_ptr()), self._stream())

    def _elem_compress(self, kind: str, x, chunk_blocks: int = 0, base=None):
        """Compress a contiguous device tensor of one of the kind's element
        widths into one frame of the kind: a uint8 device tensor of its exact
        length.  One synchronisation, to read the length."""
        t = self.torch
        w = self._elem_width(kind, x)
        self._elem_base(kind, base, x.numel(), x.dtype)
        scratch = t.empty(self._elem_scratch_bytes(kind, x.numel(), w), dtype=t.uint8, device=self.device)
        out = t.empty(self._elem_bound(kind, x.numel(), w), dtype=t.uint8, device=self.device)
        out_len = t.zeros(1, dtype=t.int64, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self._elem_compress_into(kind, x, scratch, out, out_len, result, chunk_blocks, base)
        return out[: int(out_len.item())]

    @staticmethod
    def _elem_info(kind: str, buf):
        """The read-header call of a frame of the kind given as bytes, a numpy
        array or a tensor (its first 48 bytes come to the host): (the kind's
        info, the inner frame's FrameInfo); raises FseError (BAD_FRAME)
        otherwise."""
        if hasattr(buf, "data_ptr"):  # a torch tensor
            head = buf[:48].cpu().numpy().tobytes()
        else:
            head = bytes(memoryview(buf)[:48])
        a = np.frombuffer(head, dtype=np.uint8)
        info, inner = _ELEM[kind].info(), FrameInfo()
        name = _ELEM[kind].prefix + "read_header"
        check(getattr(load(), name)(_p(a), len(a), C.byref(info), C.byref(inner)), name)
        return info, inner

    def _check_dtype(self, info, dtype, kind: str = "plane") -> None:
        w = self.torch.empty(0, dtype=dtype).element_size()
        if w != info.elem_bytes:
            raise ValueError(f"dtype {dtype} has {w}-byte elements, the {kind} frame holds {info.elem_bytes}-byte ones")

    def _elem_decompress_into(self, kind: str, buf, info, inner: FrameInfo, scratch, out, block_status, result,
                              chunk_blocks: int = 0, base=None) -> None:
        """The decompress call, no synchronisation: `scratch` >= inner.n_total
        bytes, `out` info.n_elems elements (16-byte aligned; the base itself
        for an in-place diff decode), `block_status` inner.n_blocks int32 or
        None, `result` two int32."""
        b = self._elem_base(kind, base, info.n_elems, out.dtype)
        self._elem_call(kind, "decompress", C.byref(info), C.byref(inner), chunk_blocks, C.c_void_p(buf.data_ptr()),
                        buf.numel(), C.c_void_p(scratch.data_ptr()), scratch.numel(), C.c_void_p(out.data_ptr()), *b,
                        out.numel() * out.element_size(),
                        C.c_void_p(block_status.data_ptr()) if block_status is not None else None,
                        C.c_void_p(result.data_ptr()), self._stream())

    def _elem_decompress(self, kind: str, buf, dtype, chunk_blocks: int = 0, base=None, out=None):
        """Decode a frame of the kind (a uint8 device tensor) into a 1-D
        tensor of `dtype` (`out` when given), whose size must be the frame's
        element width (ValueError otherwise).  Returns (out, block_status);
        raises FseError for a frame-level error (BAD_FRAME)."""
        t = self.torch
        info, inner = self._elem_info(kind, buf)
        self._check_dtype(info, dtype, _ELEM[kind].label)
        self._elem_base(kind, base, info.n_elems, dtype)
        scratch = t.empty(inner.n_total, dtype=t.uint8, device=self.device)
        out = self._elem_out(out, info.n_elems, dtype)
        status = t.zeros(inner.n_blocks, dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self._elem_decompress_into(kind, buf, info, inner, scratch, out, status, result, chunk_blocks, base)
        check(int(result[0].item()), f"{_ELEM[kind].label} frame")
        return out, status

    @staticmethod
    def planes_ranges(ranges):
        """(elem_off, n_elems, dst_elem_off) triples as the fsehip_planes_range array the C calls of both kinds read."""
        arr = (PlanesRange * max(len(ranges), 1))(*[PlanesRange(int(s), int(n), int(d)) for s, n, d in ranges])
        arr.empty = len(ranges) == 0
        return arr

    def _elem_ranges_scratch_bytes(self, kind: str, elem_bytes: int, ranges) -> int:
        arr = ranges if isinstance(ranges, C.Array) else self.planes_ranges(ranges)
        n = 0 if getattr(arr, "empty", False) else len(arr)
        return int(self._elem_fn(kind, "ranges_scratch_bytes")(elem_bytes, arr, n))

    def _elem_decompress_ranges_into(self, kind: str, buf, info, inner: FrameInfo, ranges, scratch, out, range_status,
                                     result, chunk_blocks: int = 0, base=None) -> None:
        """The decompress-ranges call, no synchronisation: `ranges` a sequence
        of (elem_off, n_elems, dst_elem_off) or what `planes_ranges` made of
        one; `scratch` >= the kind's ranges_scratch_bytes; range r goes to
        out[dst_elem_off: dst_elem_off + n_elems] (`out` of the frame's
        element width, any alignment; for a diff frame clear of `base`, the
        whole base tensor)."""
        arr = ranges if isinstance(ranges, C.Array) else self.planes_ranges(ranges)
        n = 0 if getattr(arr, "empty", False) else len(arr)
        b = self._elem_base(kind, base, info.n_elems, out.dtype)
        self._elem_call(kind, "decompress_ranges", C.byref(info), C.byref(inner), chunk_blocks,
                        C.c_void_p(buf.data_ptr()), buf.numel(), arr, n, C.c_void_p(scratch.data_ptr()),
                        scratch.numel(), C.c_void_p(out.data_ptr()), *b, out.numel() * out.element_size(),
                        C.c_void_p(range_status.data_ptr()) if range_status is not None else None,
                        C.c_void_p(result.data_ptr()), self._stream())

    def _elem_decompress_ranges(self, kind: str, buf, dtype, ranges, chunk_blocks: int = 0, base=None):
        """Decode the element ranges [(elem_off, count), ...] of a frame of the
        kind without decoding the rest (a delta range from its restart group's
        first element on).  The ranges are packed back to back into one
        tensor of `dtype`; returns (list of views of it, one per range, and
        the int32 range statuses).  Raises FseError for a frame-level error
        (BAD_FRAME)."""
        t = self.torch
        info, inner = self._elem_info(kind, buf)
        self._check_dtype(info, dtype, _ELEM[kind].label)
        self._elem_base(kind, base, info.n_elems, dtype)
        packed, at = [], 0
        for s, n in ranges:
            packed.append((s, n, at))
            at += n
        arr = self.planes_ranges(packed)
        scratch = t.empty(max(self._elem_ranges_scratch_bytes(kind, info.elem_bytes, arr), 16), dtype=t.uint8,
                          device=self.device)
        out = t.empty(at, dtype=dtype, device=self.device)
        status = t.zeros(len(packed), dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self._elem_decompress_ranges_into(kind, buf, info, inner, arr, scratch, out, status, result, chunk_blocks,
                                          base)
        check(int(result[0].item()), f"{_ELEM[kind].label} frame")
        return [out[d: d + n] for _, n, d in packed], status

    def _elem_decompress_range(self, kind: str, buf, dtype, elem_off: int, count: int, chunk_blocks: int = 0,
                               base=None):
        """Elements [elem_off, elem_off + count) of a frame of the kind as a
        tensor of `dtype`; raises FseError for a frame-level error or with the
        status of the first failed block the range needs."""
        views, status = self._elem_decompress_ranges(kind, buf, dtype, [(elem_off, count)], chunk_blocks, base)
        check(int(status[0].item()), f"{_ELEM[kind].label} frame range")
        return views[0]

    # the plane frame's names (2-, 4- and 8-byte elements)
    def planes_bound(self, n_elems: int, elem_bytes: int) -> int:
        """`fsehip_planes_bound`: a capacity no plane frame of n_elems elements exceeds."""
        return self._elem_bound("planes", n_elems, elem_bytes)

    def planes_scratch_bytes(self, n_elems: int, elem_bytes: int) -> int:
        """`fsehip_planes_scratch_bytes`: the plane image's bytes."""
        return self._elem_scratch_bytes("planes", n_elems, elem_bytes)

    def planes_split(self, x):
        """`fsehip_planes_split`: `_elem_split` for the plane image."""
        return self._elem_split("planes", x)

    def planes_merge(self, image, n_elems: int, dtype):
        """`fsehip_planes_merge`: `_elem_merge` from a plane image."""
        return self._elem_merge("planes", image, n_elems, dtype)

    def compress_planes_into(self, x, scratch, out, out_len, result, chunk_blocks: int = 0) -> None:
        """`fsehip_planes_compress`: `_elem_compress_into` for a plane frame."""
        self._elem_compress_into("planes", x, scratch, out, out_len, result, chunk_blocks)

    def compress_planes(self, x, chunk_blocks: int = 0):
        """`_elem_compress` into one plane frame."""
        return self._elem_compress("planes", x, chunk_blocks)

    @staticmethod
    def planes_info(buf):
        """`fsehip_planes_read_header`: `_elem_info`, (PlanesInfo, FrameInfo)."""
        return BlockCodec._elem_info("planes", buf)

    def decompress_planes_into(self, buf, info: PlanesInfo, inner: FrameInfo, scratch, out, block_status, result,
                               chunk_blocks: int = 0) -> None:
        """`fsehip_planes_decompress`: `_elem_decompress_into` for a plane frame."""
        self._elem_decompress_into("planes", buf, info, inner, scratch, out, block_status, result, chunk_blocks)

    def decompress_planes(self, buf, dtype, chunk_blocks: int = 0):
        """`_elem_decompress` of a plane frame: (out, block_status)."""
        return self._elem_decompress("planes", buf, dtype, chunk_blocks)

    def planes_ranges_scratch_bytes(self, elem_bytes: int, ranges) -> int:
        """`fsehip_planes_ranges_scratch_bytes` for a sequence of triples or a `planes_ranges` array."""
        return self._elem_ranges_scratch_bytes("planes", elem_bytes, ranges)

    def decompress_planes_ranges_into(self, buf, info: PlanesInfo, inner: FrameInfo, ranges, scratch, out,
                                      range_status, result, chunk_blocks: int = 0) -> None:
        """`fsehip_planes_decompress_ranges`: `_elem_decompress_ranges_into` for a plane frame."""
        self._elem_decompress_ranges_into("planes", buf, info, inner, ranges, scratch, out, range_status, result,
                                          chunk_blocks)

    def decompress_planes_ranges(self, buf, dtype, ranges, chunk_blocks: int = 0):
        """`_elem_decompress_ranges` of a plane frame: (views, range statuses)."""
        return self._elem_decompress_ranges("planes", buf, dtype, ranges, chunk_blocks)

    def decompress_planes_range(self, buf, dtype, elem_off: int, count: int, chunk_blocks: int = 0):
        """`_elem_decompress_range` of a plane frame: one tensor."""
        return self._elem_decompress_range("planes", buf, dtype, elem_off, count, chunk_blocks)

    # the delta frame's names (1-, 2-, 4- and 8-byte elements)
    def delta_bound(self, n_elems: int, elem_bytes: int) -> int:
        """`fsehip_delta_bound`: a capacity no delta frame of n_elems elements exceeds."""
        return self._elem_bound("delta", n_elems, elem_bytes)

    def delta_scratch_bytes(self, n_elems: int, elem_bytes: int) -> int:
        """`fsehip_delta_scratch_bytes`: the delta image's bytes."""
        return self._elem_scratch_bytes("delta", n_elems, elem_bytes)

    def delta_encode(self, x):
        """`fsehip_delta_encode`: `_elem_split` for the delta image."""
        return self._elem_split("delta", x)

    def delta_decode(self, image, n_elems: int, dtype):
        """`fsehip_delta_decode`: `_elem_merge` from a delta image."""
        return self._elem_merge("delta", image, n_elems, dtype)

    def compress_delta_into(self, x, scratch, out, out_len, result, chunk_blocks: int = 0) -> None:
        """`fsehip_delta_compress`: `_elem_compress_into` for a delta frame."""
        self._elem_compress_into("delta", x, scratch, out, out_len, result, chunk_blocks)

    def compress_delta(self, x, chunk_blocks: int = 0):
        """`_elem_compress` into one delta frame."""
        return self._elem_compress("delta", x, chunk_blocks)

    @staticmethod
    def delta_info(buf):
        """`fsehip_delta_read_header`: `_elem_info`, (DeltaInfo, FrameInfo)."""
        return BlockCodec._elem_info("delta", buf)

    def decompress_delta_into(self, buf, info: DeltaInfo, inner: FrameInfo, scratch, out, block_status, result,
                              chunk_blocks: int = 0) -> None:
        """`fsehip_delta_decompress`: `_elem_decompress_into` for a delta frame."""
        self._elem_decompress_into("delta", buf, info, inner, scratch, out, block_status, result, chunk_blocks)

    def decompress_delta(self, buf, dtype, chunk_blocks: int = 0):
        """`_elem_decompress` of a delta frame: (out, block_status)."""
        return self._elem_decompress("delta", buf, dtype, chunk_blocks)

    def delta_ranges_scratch_bytes(self, elem_bytes: int, ranges) -> int:
        """`fsehip_delta_ranges_scratch_bytes` for a sequence of triples or a `planes_ranges` array."""
        return self._elem_ranges_scratch_bytes("delta", elem_bytes, ranges)

    def decompress_delta_ranges_into(self, buf, info: DeltaInfo, inner: FrameInfo, ranges, scratch, out,
                                     range_status, result, chunk_blocks: int = 0) -> None:
        """`fsehip_delta_decompress_ranges`: `_elem_decompress_ranges_into` for a delta frame."""
        self._elem_decompress_ranges_into("delta", buf, info, inner, ranges, scratch, out, range_status, result,
                                          chunk_blocks)

    def decompress_delta_ranges(self, buf, dtype, ranges, chunk_blocks: int = 0):
        """`_elem_decompress_ranges` of a delta frame: (views, range statuses)."""
        return self._elem_decompress_ranges("delta", buf, dtype, ranges, chunk_blocks)

    def decompress_delta_range(self, buf, dtype, elem_off: int, count: int, chunk_blocks: int = 0):
        """`_elem_decompress_range` of a delta frame: one tensor."""
        return self._elem_decompress_range("delta", buf, dtype, elem_off, count, chunk_blocks)

    # the diff frame's names (1-, 2-, 4- and 8-byte elements): `base` is a
    # contiguous device tensor of the dtype and element count of `x` (decode:
    # of the header), ValueError otherwise; the decoded dtype is the base's.
    # Passing out=base decodes in place.
    @staticmethod
    def _diff_base(base):
        if base is None or not hasattr(base, "data_ptr"):
            raise ValueError("the diff frame needs its base tensor")
        return base

    def diff_bound(self, n_elems: int, elem_bytes: int) -> int:
        """`fsehip_diff_bound`: a capacity no diff frame of n_elems elements exceeds."""
        return self._elem_bound("diff", n_elems, elem_bytes)

    def diff_scratch_bytes(self, n_elems: int, elem_bytes: int) -> int:
        """`fsehip_diff_scratch_bytes`: the diff image's bytes."""
        return self._elem_scratch_bytes("diff", n_elems, elem_bytes)

    def diff_encode(self, x, base):
        """`fsehip_diff_encode`: `_elem_split` for the diff image of `x` against `base`."""
        return self._elem_split("diff", x, base)

    def diff_decode(self, image, base, out=None):
        """`fsehip_diff_decode`: `_elem_merge` from a diff image against
        `base`, into a fresh tensor, `out`, or the base itself (out=base)."""
        base = self._diff_base(base)
        return self._elem_merge("diff", image, base.numel(), base.dtype, base, out)

    def compress_diff_into(self, x, base, scratch, out, out_len, result, chunk_blocks: int = 0) -> None:
        """`fsehip_diff_compress`: `_elem_compress_into` for a diff frame."""
        self._elem_compress_into("diff", x, scratch, out, out_len, result, chunk_blocks, base)

    def compress_diff(self, x, base, chunk_blocks: int = 0):
        """`_elem_compress` into one diff frame of `x` against `base`."""
        return self._elem_compress("diff", x, chunk_blocks, base)

    @staticmethod
    def diff_info(buf):
        """`fsehip_diff_read_header`: `_elem_info`, (DiffInfo, FrameInfo)."""
        return BlockCodec._elem_info("diff", buf)

    def decompress_diff_into(self, buf, info: DiffInfo, inner: FrameInfo, base, scratch, out, block_status, result,
                             chunk_blocks: int = 0) -> None:
        """`fsehip_diff_decompress`: `_elem_decompress_into` for a diff frame (out may be the base)."""
        self._elem_decompress_into("diff", buf, info, inner, scratch, out, block_status, result, chunk_blocks, base)

    def decompress_diff(self, buf, base, out=None, chunk_blocks: int = 0):
        """`_elem_decompress` of a diff frame against `base`: (out,
        block_status), out of the base's dtype; out=base updates the base
        where it lies.  The frame does not identify its base: another one
        decodes to other values with every status OK (compress_sealed(kind=
        "diff") adds checksums that tell)."""
        return self._elem_decompress("diff", buf, self._diff_base(base).dtype, chunk_blocks, base, out)

    def diff_ranges_scratch_bytes(self, elem_bytes: int, ranges) -> int:
        """`fsehip_diff_ranges_scratch_bytes` for a sequence of triples or a `planes_ranges` array."""
        return self._elem_ranges_scratch_bytes("diff", elem_bytes, ranges)

    def decompress_diff_ranges_into(self, buf, info: DiffInfo, inner: FrameInfo, ranges, base, scratch, out,
                                    range_status, result, chunk_blocks: int = 0) -> None:
        """`fsehip_diff_decompress_ranges`: `_elem_decompress_ranges_into` for
        a diff frame; `base` is the whole base tensor and `out` lies clear of it."""
        self._elem_decompress_ranges_into("diff", buf, info, inner, ranges, scratch, out, range_status, result,
                                          chunk_blocks, base)

    def decompress_diff_ranges(self, buf, base, ranges, chunk_blocks: int = 0):
        """`_elem_decompress_ranges` of a diff frame against the whole base: (views, range statuses)."""
        return self._elem_decompress_ranges("diff", buf, self._diff_base(base).dtype, ranges, chunk_blocks, base)

    def decompress_diff_range(self, buf, base, elem_off: int, count: int, chunk_blocks: int = 0):
        """`_elem_decompress_range` of a diff frame against the whole base: one tensor."""
        return self._elem_decompress_range("diff", buf, self._diff_base(base).dtype, elem_off, count, chunk_blocks,
                                           base)

    # ------------------------------------------------------------ the check record and sealed buffers
    # fsehip.h section 2f: a CRC-32 (zlib's) per check block of the content,
    # in a record of its own in front of an unchanged container.
    @staticmethod
    def _check_log(check_block: int) -> int:
        log = int(check_block).bit_length() - 1
        if check_block != 1 << log or not 8 <= log <= 16:
            raise ValueError(f"check_block {check_block}: a power of two from 256 to 65536")
        return log

    @staticmethod
    def _content_bytes(x) -> int:
        if not x.is_contiguous():
            raise ValueError("the check record needs a contiguous tensor")
        return x.numel() * x.element_size()

    def check_bytes(self, n_content: int, check_block: int = 65536) -> int:
        """`fsehip_check_bytes`: the record's size for n_content bytes."""
        return int(self.lib.fsehip_check_bytes(n_content, self._check_log(check_block)))

    def check_build_into(self, x, record, check_block: int = 65536) -> None:
        """`fsehip_check_build`, no synchronisation: the record of the bytes of
        `x` (any contiguous tensor, any alignment) into `record`, a uint8
        device tensor of check_bytes (any alignment)."""
        n = self._content_bytes(x)
        if record.numel() < self.check_bytes(n, check_block):
            raise FseError(-7, "fsehip_check_build")
        check(self.lib.fsehip_check_build(self._check_log(check_block), C.c_void_p(x.data_ptr()), n,
                                          C.c_void_p(record.data_ptr()), self._stream()), "fsehip_check_build")

    def check_build(self, x, check_block: int = 65536):
        """The check record of a contiguous device tensor's bytes: a uint8 device tensor."""
        record = self.torch.empty(self.check_bytes(self._content_bytes(x), check_block), dtype=self.torch.uint8,
                                  device=self.device)
        self.check_build_into(x, record, check_block)
        return record

    @staticmethod
    def check_info(record) -> CheckInfo:
        """`fsehip_check_read_header` of a record given as bytes, a numpy array
        or a tensor (its first 32 bytes come to the host); raises FseError
        (BAD_FRAME) for anything that is not a check record's header."""
        if hasattr(record, "data_ptr"):  # a torch tensor
            head = record[:32].cpu().numpy().tobytes()
        else:
            head = bytes(memoryview(record)[:32])
        a = np.frombuffer(head, dtype=np.uint8)
        info = CheckInfo()
        check(load().fsehip_check_read_header(_p(a), len(a), C.byref(info)), "fsehip_check_read_header")
        return info

    def check_verify_into(self, record, info: CheckInfo, x, check_status, result) -> None:
        """`fsehip_check_verify`, no synchronisation: `check_status` info.n_cb
        int32, `result` two int32 (OK / CHECKSUM of the whole content / BAD_FRAME,
        failed check blocks)."""
        check(self.lib.fsehip_check_verify(
            C.byref(info), C.c_void_p(record.data_ptr()), C.c_void_p(x.data_ptr()), self._content_bytes(x),
            C.c_void_p(check_status.data_ptr()), C.c_void_p(result.data_ptr()), self._stream()), "fsehip_check_verify")

    def check_verify(self, record, x):
        """Compare a record (a uint8 device tensor) with the bytes of `x`:
        (check_status, result), both int32 device tensors."""
        t = self.torch
        info = self.check_info(record)
        status = t.zeros(info.n_cb, dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self.check_verify_into(record, info, x, status, result)
        return status, result

    def check_ranges_verified_bytes(self, info: CheckInfo, ranges) -> int:
        """`fsehip_check_ranges_verified_bytes`: the bytes of the byte ranges
        (src_off, len, dst_off) that lie in wholly covered check blocks."""
        arr = ranges if isinstance(ranges, C.Array) else self.frame_ranges(ranges)
        n = 0 if getattr(arr, "empty", False) else len(arr)
        out = C.c_uint64(0)
        check(self.lib.fsehip_check_ranges_verified_bytes(C.byref(info), arr, n, C.byref(out)),
              "fsehip_check_ranges_verified_bytes")
        return int(out.value)

    def check_verify_ranges_into(self, record, info: CheckInfo, ranges, out, range_status, result) -> None:
        """`fsehip_check_verify_ranges`, no synchronisation: `ranges` byte
        triples (src_off, len, dst_off) or a `frame_ranges` array, range r's
        bytes at byte dst_off of `out` (any tensor, any alignment);
        `range_status` len(ranges) int32, `result` two int32."""
        arr = ranges if isinstance(ranges, C.Array) else self.frame_ranges(ranges)
        n = 0 if getattr(arr, "empty", False) else len(arr)
        check(self.lib.fsehip_check_verify_ranges(
            C.byref(info), C.c_void_p(record.data_ptr()), arr, n, C.c_void_p(out.data_ptr()),
            out.numel() * out.element_size(), C.c_void_p(range_status.data_ptr()), C.c_void_p(result.data_ptr()),
            self._stream()), "fsehip_check_verify_ranges")

    def _sealed_kind(self, x, kind: str) -> int:
        if kind == "frame":
            if x.element_size() != 1:
                raise ValueError("a sealed frame takes a 1-byte tensor; wider elements go to kind='planes' or 'delta'")
            return 1
        if kind not in _ELEM:
            raise ValueError(f"kind {kind!r}: 'frame', 'planes', 'delta' or 'diff'")
        return self._elem_width(kind, x)

    @staticmethod
    def _sealed_candidates(x, base=None) -> tuple:
        """What kind='auto' chooses among: a sealed frame takes 1-byte tensors
        only, a plane frame wider ones only, a diff frame needs the base."""
        return ("frame" if x.element_size() == 1 else "planes", "delta") + (("diff",) if base is not None else ())

    def sealed_bound(self, x, kind: str = "frame", check_block: int = 65536) -> int:
        """A capacity no sealed buffer of `x` exceeds: the record, then the
        container's bound; for kind 'auto' the largest of the candidates'."""
        if kind == "auto":
            return max(self.sealed_bound(x, k, check_block) for k in self._sealed_candidates(x) + ("diff",))
        w = self._sealed_kind(x, kind)
        inner = self.frame_bound(x.numel()) if kind == "frame" else self._elem_bound(kind, x.numel(), w)
        return self.check_bytes(self._content_bytes(x), check_block) + inner

    def compress_sealed_into(self, x, kind, buf, out_len, result, scratch=None, check_block: int = 65536,
                             chunk_blocks: int = 0, base=None) -> int:
        """The record of `x` at buf[0], then the existing compress_*_into
        straight to the record's end: no synchronisation, no copy of the
        container.  `buf` >= sealed_bound bytes, `out_len` one int64 (the
        CONTAINER's length), `result` two int32, `scratch` as the plane,
        delta or diff call's, `base` for kind 'diff' alone.  Returns the
        record's size: the buffer's length is that plus out_len."""
        self._sealed_kind(x, kind)
        if kind == "frame":
            if base is not None:
                raise ValueError("a sealed frame takes no base")
        else:
            self._elem_base(kind, base, x.numel(), x.dtype)
        rec = self.check_bytes(self._content_bytes(x), check_block)
        self.check_build_into(x, buf[:rec], check_block)
        if kind == "frame":
            self.compress_frame_into(x, buf[rec:], out_len, result, chunk_blocks)
        else:
            self._elem_compress_into(kind, x, scratch, buf[rec:], out_len, result, chunk_blocks, base)
        return rec

    def compress_sealed(self, x, kind: str = "frame", check_block: int = 65536, chunk_blocks: int = 0, base=None):
        """Compress a contiguous device tensor into one sealed buffer (a check
        record, then a frame, plane frame, delta frame or -- kind 'diff',
        against `base` -- diff frame): a uint8 device tensor of its exact
        length.  One synchronisation, to read the length.  kind 'auto'
        estimates first (one more synchronisation) and seals the kind
        `estimate_choose` picks among the frame (1-byte tensors), the plane
        frame (wider ones), the delta frame and, with `base`, the diff frame:
        the buffer is compress_sealed's of that kind, which sealed_info names."""
        t = self.torch
        if kind == "auto":
            if base is not None:
                self._elem_base("diff", base, x.numel(), x.dtype)
            kind = estimate_choose(self.estimate(x, self._sealed_candidates(x, base), base))
            base = base if kind == "diff" else None
        w = self._sealed_kind(x, kind)
        scratch = None
        if kind != "frame":
            scratch = t.empty(self._elem_scratch_bytes(kind, x.numel(), w), dtype=t.uint8, device=self.device)
        buf = t.empty(self.sealed_bound(x, kind, check_block), dtype=t.uint8, device=self.device)
        out_len = t.zeros(1, dtype=t.int64, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        rec = self.compress_sealed_into(x, kind, buf, out_len, result, scratch, check_block, chunk_blocks, base)
        return buf[: rec + int(out_len.item())]

    @staticmethod
    def sealed_info(buf):
        """`fsehip_sealed_read_header` of a sealed buffer given as bytes, a
        numpy array or a tensor (the record and the container's first 48 bytes
        come to the host): (CheckInfo, kind, inner_off) with kind 'frame',
        'planes', 'delta' or 'diff' and the container at buf[inner_off:]; raises
        FseError (BAD_FRAME) otherwise."""
        info = BlockCodec.check_info(buf)
        upto = 32 + 4 * info.n_cb + 48
        if hasattr(buf, "data_ptr"):  # a torch tensor
            head = buf[:upto].cpu().numpy().tobytes()
        else:
            head = bytes(memoryview(buf)[:upto])
        a = np.frombuffer(head, dtype=np.uint8)
        kind, off = C.c_uint32(0), C.c_uint64(0)
        check(load().fsehip_sealed_read_header(_p(a), len(a), C.byref(info), C.byref(kind), C.byref(off)),
              "fsehip_sealed_read_header")
        return info, SEALED_KINDS[kind.value], int(off.value)

    def _sealed_dtype(self, kind: str, inner, dtype):
        """The dtype a sealed buffer decodes to: uint8 for a frame, `dtype`
        (default: the integer of the container's element width) otherwise."""
        t = self.torch
        if kind == "frame":
            if dtype is not None and t.empty(0, dtype=dtype).element_size() != 1:
                raise ValueError(f"dtype {dtype}: a sealed frame holds bytes")
            return dtype or t.uint8
        return dtype or {1: t.uint8, 2: t.int16, 4: t.int32, 8: t.int64}[self._elem_info(kind, inner)[0].elem_bytes]

    def sealed_inner_info(self, kind: str, inner):
        """The container's own header(s) at the start of `inner` (bytes, numpy
        or a tensor): FrameInfo for a frame, (PlanesInfo | DeltaInfo,
        FrameInfo) otherwise."""
        return self.frame_info(inner) if kind == "frame" else self._elem_info(kind, inner)

    def decompress_sealed_into(self, buf, sealed, inner_info, out, block_status, result, check_status, check_result,
                               scratch=None, chunk_blocks: int = 0, base=None) -> None:
        """The existing decompress_*_into of the container, then
        `fsehip_check_verify` on the output; no synchronisation.  `sealed` is
        what sealed_info gave for the buffer, `inner_info` what
        sealed_inner_info gave for its container; `out`, `block_status`,
        `result`, `scratch` and `base` (a diff frame's) as the container's
        call, `check_status` sealed[0].n_cb int32, `check_result` two int32."""
        info, kind, off = sealed
        inner = buf[off:]
        if kind == "frame":
            self.decompress_frame_into(inner, inner_info, out, block_status, result, chunk_blocks)
        else:
            self._elem_decompress_into(kind, inner, *inner_info, scratch, out, block_status, result, chunk_blocks,
                                       base)
        self.check_verify_into(buf, info, out, check_status, check_result)

    def _sealed_base(self, kind: str, base, dtype):
        """`base` belongs to a sealed diff buffer and to no other; its dtype is
        the default one there.  Returns the dtype to decode to."""
        if kind == "diff":
            if base is None:
                raise ValueError("a sealed diff buffer needs base=")
            return dtype or self._diff_base(base).dtype
        if base is not None:
            raise ValueError(f"a sealed {kind} buffer takes no base")
        return dtype

    def decompress_sealed(self, buf, dtype=None, chunk_blocks: int = 0, with_result: bool = False, base=None):
        """Decode a sealed buffer (a uint8 device tensor) with the existing
        decompress of its container, then verify the output against the
        record: (out, block_status, check_status), or with_result=True
        (out, block_status, check_status, result) with the verify's two int32
        (result[0]: OK, CHECKSUM of the whole content; result[1]: failed check
        blocks).  A sealed diff buffer needs `base` (dtype defaults to the
        base's), and a wrong base shows as CHECKSUM in the check blocks it
        changes.  Raises FseError for a buffer-level error (BAD_FRAME)."""
        t = self.torch
        sealed = info, kind, off = self.sealed_info(buf)
        inner_info = self.sealed_inner_info(kind, buf[off:])
        dtype = self._sealed_base(kind, base, dtype)
        dt = self._sealed_dtype(kind, buf[off:], dtype)
        scratch = None
        if kind == "frame":
            finfo = inner_info
            out = t.empty(info.n_content, dtype=dt, device=self.device)
        else:
            self._check_dtype(inner_info[0], dt, _ELEM[kind].label)
            self._elem_base(kind, base, inner_info[0].n_elems, dt)
            finfo = inner_info[1]
            scratch = t.empty(finfo.n_total, dtype=t.uint8, device=self.device)
            out = t.empty(inner_info[0].n_elems, dtype=dt, device=self.device)
        block_status = t.zeros(finfo.n_blocks, dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        check_status = t.zeros(info.n_cb, dtype=t.int32, device=self.device)
        check_result = t.zeros(2, dtype=t.int32, device=self.device)
        self.decompress_sealed_into(buf, sealed, inner_info, out, block_status, result, check_status, check_result,
                                    scratch, chunk_blocks, base)
        check(int(result[0].item()), f"sealed {kind}")
        if int(check_result[0].item()) == -19:  # the record on the device is not the one the host read
            raise FseError(-19, "check record")
        if with_result:
            return out, block_status, check_status, check_result
        return out, block_status, check_status

    def decompress_sealed_ranges(self, buf, dtype, ranges, chunk_blocks: int = 0, base=None):
        """Decode the ranges [(off, count), ...] of a sealed buffer without
        decoding the rest -- elements of `dtype` when the container is a plane,
        delta or diff frame (the last against `base`, the whole base tensor),
        bytes (dtype None or a 1-byte one) for a frame -- and
        verify the check blocks each range wholly covers.  Returns (views, one
        per range, of one packed tensor; the container's range statuses; the
        check's range statuses, OK or CHECKSUM).  Raises FseError for a
        buffer-level error (BAD_FRAME)."""
        t = self.torch
        info, kind, off = self.sealed_info(buf)
        inner = buf[off:]
        dt = self._sealed_dtype(kind, inner, self._sealed_base(kind, base, dtype))
        w = t.empty(0, dtype=dt).element_size()
        packed, at = [], 0
        for s, n in ranges:
            packed.append((s, n, at))
            at += n
        out = t.empty(at, dtype=dt, device=self.device)
        status = t.zeros(len(packed), dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        if kind == "frame":
            self.decompress_frame_ranges_into(inner, self.frame_info(inner), packed, out, status, result, chunk_blocks)
        else:
            pinfo, finfo = self._elem_info(kind, inner)
            self._check_dtype(pinfo, dt, _ELEM[kind].label)
            arr = self.planes_ranges(packed)
            scratch = t.empty(max(self._elem_ranges_scratch_bytes(kind, w, arr), 16), dtype=t.uint8, device=self.device)
            self._elem_decompress_ranges_into(kind, inner, pinfo, finfo, arr, scratch, out, status, result,
                                              chunk_blocks, base)
        check(int(result[0].item()), f"sealed {kind}")
        check_status = t.zeros(len(packed), dtype=t.int32, device=self.device)
        check_result = t.zeros(2, dtype=t.int32, device=self.device)
        self.check_verify_ranges_into(buf, info, [(s * w, n * w, d * w) for s, n, d in packed], out, check_status,
                                      check_result)
        check(int(check_result[0].item()), "check record")
        return [out[d: d + n] for _, n, d in packed], status, check_status

    def decompress_sealed_range(self, buf, dtype, off: int, count: int, chunk_blocks: int = 0, base=None):
        """One range of a sealed buffer as a tensor; raises FseError for a
        buffer-level error, with the status of the first failed block the
        range touches, or with CHECKSUM when a check block the range wholly
        covers fails."""
        views, status, check_status = self.decompress_sealed_ranges(buf, dtype, [(off, count)], chunk_blocks, base)
        check(int(status[0].item()), "sealed range")
        check(int(check_status[0].item()), "sealed range")
        return views[0]

    # ------------------------------------------------------------ the size estimate
    # fsehip.h sections 2g and 2i: the length each container would have, from
    # the block histograms of its image and the encoder's own normalisation,
    # and the automatic choice among compress_frame / compress_planes /
    # compress_delta and, for a caller who passes the tensor's base,
    # compress_diff.  Kinds are "frame", "planes", "delta" (or 0, 1, 2) and,
    # with base=, "diff" (or 4).
    @staticmethod
    def _kind(kind, base=None) -> int:
        k = KINDS.index(kind) if isinstance(kind, str) and kind in KINDS else kind
        if base is not None and kind in ("diff", KIND_DIFF):
            return KIND_DIFF
        if k not in (0, 1, 2):
            if kind in ("diff", KIND_DIFF):
                raise ValueError("kind 'diff' estimates against a base: pass base=")
            raise ValueError(f"kind {kind!r}: one of {KINDS}" + (" or 'diff'" if base is not None else ""))
        return k

    @staticmethod
    def _estimate_elem_bytes(x) -> int:
        w = x.element_size()
        if w not in (1, 2, 4, 8):
            raise ValueError(f"element size {w}: the containers take 1, 2, 4 or 8 bytes")
        if not x.is_contiguous():
            raise ValueError("the estimate needs a contiguous tensor")
        return w

    def _kind_mask(self, kinds, base=None) -> int:
        """Bit k for every kind asked for (None: all three, and with a base
        the diff frame); a kind that does not take the width stays in the mask
        and is estimated as EST_NONE."""
        mask = 0
        for kind in (KINDS + (("diff",) if base is not None else ()) if kinds is None else kinds):
            mask |= 1 << self._kind(kind, base)
        if mask == 0:
            raise ValueError("no kind asked for")
        return mask

    @staticmethod
    def _estimate_base(x, base):
        """The base of an estimate after its checks (ValueError): a contiguous
        device tensor of x's element width and element count."""
        if not hasattr(base, "data_ptr") or not base.is_cuda:
            raise ValueError("base must be a device tensor")
        if not base.is_contiguous():
            raise ValueError("base must be contiguous")
        if base.element_size() != x.element_size() or base.numel() != x.numel():
            raise ValueError(f"base has {base.numel()} elements of {base.element_size()} bytes, the tensor "
                             f"{x.numel()} of {x.element_size()}")
        return C.c_void_p(base.data_ptr())

    def _frame_params(self, chunk_blocks: int = 0) -> FrameParams:
        return FrameParams(self.block_size, self.table_log, self.ckpt_interval, self.max_table_log, self.nstates,
                           chunk_blocks)

    def image_histogram(self, x, kind, base=None):
        """`fsehip_image_histogram`: the 256-bin byte counts of every block
        (the codec's block size) of the image the container of `kind` codes
        for the contiguous device tensor x -- its raw bytes, its plane image
        or its delta image, or (`fsehip_diff_image_histogram`, kind "diff")
        its diff image against `base` -- the images themselves never written.
        A uint32 device tensor [n_blocks, 256]; no synchronisation."""
        t = self.torch
        w, k = self._estimate_elem_bytes(x), self._kind(kind, base)
        n_image = int(self.lib.fsehip_estimate_image_bytes(2 if k == KIND_DIFF else k, x.numel(), w))
        counts = t.zeros((self.n_blocks(n_image), 256), dtype=t.int32, device=self.device).view(t.uint32)
        if k == KIND_DIFF:
            check(self.lib.fsehip_diff_image_histogram(
                w, C.c_void_p(x.data_ptr()), self._estimate_base(x, base), x.numel(), self.block_size,
                C.c_void_p(counts.data_ptr()), self._stream()), "fsehip_diff_image_histogram")
            return counts
        check(self.lib.fsehip_image_histogram(k, w, C.c_void_p(x.data_ptr()), x.numel(), self.block_size,
                                              C.c_void_p(counts.data_ptr()), self._stream()), "fsehip_image_histogram")
        return counts

    def estimate_blocks(self, counts, n_image: int) -> dict:
        """`fsehip_estimate_blocks` for a [n_blocks, 256] uint32 (or int32)
        device tensor of counts of an image of n_image bytes, under the
        codec's table log, checkpoint interval and nstates: device tensors
        `type` (uint8: 0 RAW, 1 RLE, 2 FSE), `rec` (int32 record bytes),
        `bits` (int32 payload bits), `log` (uint8) per block and `total` (one
        int64: the frame's estimated length).  No synchronisation."""
        t = self.torch
        nb = self.n_blocks(n_image)
        out = {"type": t.zeros(nb, dtype=t.uint8, device=self.device),
               "rec": t.zeros(nb, dtype=t.int32, device=self.device),
               "bits": t.zeros(nb, dtype=t.int32, device=self.device),
               "log": t.zeros(nb, dtype=t.uint8, device=self.device),
               "total": t.zeros(1, dtype=t.int64, device=self.device)}
        p = self._frame_params()
        check(self.lib.fsehip_estimate_blocks(
            C.byref(p), C.c_void_p(counts.data_ptr()), n_image, C.c_void_p(out["type"].data_ptr()),
            C.c_void_p(out["rec"].data_ptr()), C.c_void_p(out["bits"].data_ptr()), C.c_void_p(out["log"].data_ptr()),
            C.c_void_p(out["total"].data_ptr()), self._stream()), "fsehip_estimate_blocks")
        return out

    def estimate_scratch_bytes(self, x, kinds=None, base=None) -> int:
        """`fsehip_estimate_scratch_bytes` for x and the kinds asked for; with
        a base `fsehip_estimate_base_scratch_bytes`."""
        w = self._estimate_elem_bytes(x)
        if base is not None:
            self._estimate_base(x, base)
            return int(self.lib.fsehip_estimate_base_scratch_bytes(x.numel(), w, self._kind_mask(kinds, base),
                                                                   self.block_size))
        return int(self.lib.fsehip_estimate_scratch_bytes(x.numel(), w, self._kind_mask(kinds), self.block_size))

    def estimate_into(self, x, scratch, est, kinds=None, base=None) -> None:
        """`fsehip_estimate`, no synchronisation: `scratch` a uint8 device
        tensor of >= estimate_scratch_bytes (16-byte aligned), `est` three
        int64 on the device, est[k] = the estimated length of kind k or -1
        (FSEHIP_EST_NONE read as int64) for a kind not asked for or not
        taking the element width.  With a base `fsehip_estimate_base`: `est`
        FIVE int64, est[3] always -1, est[4] the diff frame's against `base`."""
        w = self._estimate_elem_bytes(x)
        p = self._frame_params()
        if base is not None:
            if est.numel() < 5:
                raise ValueError("with a base the estimate writes five int64")
            check(self.lib.fsehip_estimate_base(
                C.byref(p), self._kind_mask(kinds, base), w, C.c_void_p(x.data_ptr()), self._estimate_base(x, base),
                x.numel(), C.c_void_p(scratch.data_ptr()), scratch.numel(), C.c_void_p(est.data_ptr()),
                self._stream()), "fsehip_estimate_base")
            return
        check(self.lib.fsehip_estimate(
            C.byref(p), self._kind_mask(kinds), w, C.c_void_p(x.data_ptr()), x.numel(),
            C.c_void_p(scratch.data_ptr()), scratch.numel(), C.c_void_p(est.data_ptr()), self._stream()),
            "fsehip_estimate")

    def estimate(self, x, kinds=None, base=None) -> dict:
        """The estimated container length of a contiguous device tensor for
        each kind of `kinds` (None: all that take its element width): a dict
        kind name -> bytes, under the codec's block size, table log,
        checkpoint interval and nstates.  One synchronisation: the 24-byte
        copy of the three estimates to the host.  With `base`, a contiguous
        device tensor of x's element width and count (ValueError otherwise),
        "diff" -- the diff frame of x against it -- is a fourth kind and among
        the default ones; the copy is 40 bytes."""
        t = self.torch
        scratch = t.empty(max(self.estimate_scratch_bytes(x, kinds, base), 16), dtype=t.uint8, device=self.device)
        est = t.zeros(3 if base is None else 5, dtype=t.int64, device=self.device)
        self.estimate_into(x, scratch, est, kinds, base)
        host = est.cpu().numpy().view(np.uint64)
        names = KINDS if base is None else _BASE_KINDS
        return {name: int(host[k]) for k, name in enumerate(names) if name and int(host[k]) != EST_NONE}

    def compress_auto(self, x, kinds=None, chunk_blocks: int = 0, base=None):
        """Estimate, choose (`estimate_choose`: the smallest, ties to frame,
        then planes, then delta, then diff) and compress: (buf, kind name),
        buf exactly what compress_frame / compress_planes / compress_delta
        returns for that kind -- or, with `base` (a contiguous device tensor
        of x's dtype and element count), compress_diff(x, base), which wins
        only when strictly smaller: it needs the base to decode.  The frame
        codes the tensor's bytes.  Two synchronisations: the estimate's and
        the length's."""
        if base is not None:
            self._elem_base("diff", base, x.numel(), x.dtype)
        est = self.estimate(x, kinds, base)
        kind = estimate_choose(est)
        if kind == "frame":
            t = self.torch  # (an empty tensor has no stride to view through)
            raw = x.reshape(-1).view(t.uint8) if x.numel() else t.empty(0, dtype=t.uint8, device=self.device)
            return self.compress_frame(raw, chunk_blocks), kind
        return self._elem_compress(kind, x, chunk_blocks, base if kind == "diff" else None), kind

    def decompress_auto(self, buf, dtype, chunk_blocks: int = 0, base=None):
        """Decode a frame, plane frame, delta frame or diff frame (a uint8
        device tensor) by its magic into a 1-D tensor of `dtype`: (out,
        block_status) as decompress_frame / decompress_planes /
        decompress_delta / decompress_diff.  A frame's bytes are viewed as
        `dtype` (ValueError when they are no whole number of elements).  A
        diff frame needs `base` (ValueError without); the others ignore it."""
        kind = container_kind(buf)
        if kind == "diff" and base is None:
            raise ValueError("a diff frame decodes against its base: pass base=")
        if kind in _ELEM:
            return self._elem_decompress(kind, buf, dtype, chunk_blocks, base if kind == "diff" else None)
        if kind in ("pack", "vpack"):
            raise ValueError("a pack frame holds many tensors and goes to decompress_pack")
        if kind != "frame":
            raise ValueError("a sealed buffer goes to decompress_sealed")
        out, status = self.decompress_frame(buf, chunk_blocks)
        w = self.torch.empty(0, dtype=dtype).element_size()
        if out.numel() % w:
            raise ValueError(f"the frame holds {out.numel()} bytes, no whole number of {dtype} elements")
        if out.numel() == 0:
            return self.torch.empty(0, dtype=dtype, device=self.device), status
        return out.view(dtype), status

    # ---- the pack frame (fsehip.h section 2j): many tensors in one container,
    # one transform launch over all of them each way around one frame call.
    # A member is coded as "planes" or "delta" (both at 1-, 2-, 4- and 8-byte
    # elements); dtypes and shapes stay with the caller.
    #
    # With bases= the same calls write and read the versioned pack (section
    # 2k): a member with a base may be coded as "diff", its zigzag difference
    # against the base tensor.  THE CONTAINER DOES NOT IDENTIFY ITS BASES.
    _PACK_KINDS = {"planes": 1, "delta": 2}
    _VPACK_KINDS = {"planes": 1, "delta": 2, "diff": KIND_DIFF}

    def _pack_fn(self, name: str, versioned: bool):
        return getattr(self.lib, ("fsehip_vpack_" if versioned else "fsehip_pack_") + name)

    def pack_bases(self, tensors, bases, kinds=None):
        """The kinds and the host array of base pointers of a versioned pack's
        list: `bases` one entry per tensor, None or a contiguous device tensor
        of the tensor's element size and count.  `kinds`: None ("diff" where a
        base is given, "planes" where not), one name or one per tensor; "diff"
        without a base is a ValueError.  Returns (names, pointer array)."""
        n = len(tensors)
        bases = list(bases)
        if len(bases) != n:
            raise ValueError(f"{len(bases)} bases for {n} tensors")
        if kinds is None:
            names = ["planes" if b is None else "diff" for b in bases]
        else:
            names = [kinds] * n if isinstance(kinds, str) else list(kinds)
        if len(names) != n:
            raise ValueError(f"{len(names)} kinds for {n} tensors")
        arr = (C.c_void_p * max(n, 1))()
        for m, (x, b, kind) in enumerate(zip(tensors, bases, names)):
            if kind == "diff" and b is None:
                raise ValueError(f"member {m}: a 'diff' member needs its base")
            if b is None:
                continue
            if not hasattr(b, "data_ptr") or not b.is_cuda or not b.is_contiguous():
                raise ValueError(f"base {m}: a versioned pack takes contiguous device tensors")
            if b.element_size() != x.element_size() or b.numel() != x.numel():
                raise ValueError(f"base {m}: {b.numel()} elements of {b.element_size()} bytes against "
                                 f"{x.numel()} of {x.element_size()}")
            arr[m] = b.data_ptr() if b.numel() else None
        return names, arr

    def pack_members(self, tensors, kinds=None, versioned: bool = False):
        """The fsehip_pack_member array of a list of contiguous device tensors.
        `kinds`: None (all "planes"), one name or one name per tensor;
        `versioned`: the list of a versioned pack, which also takes "diff"."""
        n = len(tensors)
        names = ["planes"] * n if kinds is None else [kinds] * n if isinstance(kinds, str) else list(kinds)
        if len(names) != n:
            raise ValueError(f"{len(names)} kinds for {n} tensors")
        arr = (PackMember * max(n, 1))()
        known = self._VPACK_KINDS if versioned else self._PACK_KINDS
        for m, (x, kind) in enumerate(zip(tensors, names)):
            if kind not in known:
                if versioned:
                    raise ValueError(f"member kind {kind!r}: a versioned pack takes 'planes', 'delta' and 'diff' members")
                raise ValueError(f"member kind {kind!r}: a pack takes 'planes' and 'delta' members")
            if not hasattr(x, "data_ptr") or not x.is_cuda or not x.is_contiguous():
                raise ValueError(f"member {m}: a pack takes contiguous device tensors")
            if x.element_size() not in (1, 2, 4, 8):
                raise ValueError(f"member {m}: element size {x.element_size()}: a pack takes 1, 2, 4 or 8 bytes")
            arr[m] = PackMember(x.data_ptr() if x.numel() else None, x.numel(), x.element_size(), known[kind])
        return arr

    def pack_bound(self, members, n: int, versioned: bool = False) -> int:
        return int(self._pack_fn("bound", versioned)(members, n, self.block_size))

    def pack_scratch_bytes(self, members, n: int, versioned: bool = False) -> int:
        return int(self._pack_fn("scratch_bytes", versioned)(members, n))

    def pack_members_scratch_bytes(self, members, n: int, indices, versioned: bool = False) -> int:
        sel = (C.c_uint32 * max(len(indices), 1))(*indices)
        return int(self._pack_fn("members_scratch_bytes", versioned)(members, n, sel, len(indices)))

    def _pack_transform_scratch(self, members, n: int, versioned: bool = False):
        t = self.torch
        extra = self.pack_scratch_bytes(members, n, versioned) - int(self._pack_fn("image_bytes", versioned)(members, n))
        return t.empty(max(extra, 16), dtype=t.uint8, device=self.device)

    def pack_split(self, tensors, kinds=None, bases=None):
        """The pack image of a list of tensors (uint8, pads zeroed):
        fsehip_pack_split; with `bases` (pack_bases) the versioned pack's,
        fsehip_vpack_split."""
        t = self.torch
        n, versioned = len(tensors), bases is not None
        if versioned:
            kinds, barr = self.pack_bases(tensors, bases, kinds)
        members = self.pack_members(tensors, kinds, versioned)
        image = t.empty(int(self._pack_fn("image_bytes", versioned)(members, n)), dtype=t.uint8, device=self.device)
        scratch = self._pack_transform_scratch(members, n, versioned)
        if versioned:
            check(self.lib.fsehip_vpack_split(members, n, barr, C.c_void_p(image.data_ptr()),
                                              C.c_void_p(scratch.data_ptr()), scratch.numel(), self._stream()),
                  "fsehip_vpack_split")
        else:
            check(self.lib.fsehip_pack_split(members, n, C.c_void_p(image.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                             scratch.numel(), self._stream()), "fsehip_pack_split")
        return image

    def pack_merge(self, image, outs, kinds=None, bases=None):
        """The members of a pack image into the tensors `outs` (their sizes
        and dtypes say the list): fsehip_pack_merge; with `bases` the
        versioned pack's, fsehip_vpack_merge (an out may be its base itself)."""
        n, versioned = len(outs), bases is not None
        if versioned:
            kinds, barr = self.pack_bases(outs, bases, kinds)
        members = self.pack_members(outs, kinds, versioned)
        scratch = self._pack_transform_scratch(members, n, versioned)
        if versioned:
            check(self.lib.fsehip_vpack_merge(members, n, barr, C.c_void_p(image.data_ptr()),
                                              C.c_void_p(scratch.data_ptr()), scratch.numel(), self._stream()),
                  "fsehip_vpack_merge")
        else:
            check(self.lib.fsehip_pack_merge(members, n, C.c_void_p(image.data_ptr()), C.c_void_p(scratch.data_ptr()),
                                             scratch.numel(), self._stream()), "fsehip_pack_merge")
        return outs

    def compress_pack_into(self, members, n: int, scratch, out, out_len, result, chunk_blocks: int = 0,
                           bases=None) -> None:
        """fsehip_pack_compress, no synchronisation: `members` from
        pack_members, `scratch` a uint8 device tensor of >= pack_scratch_bytes
        (16-byte aligned), `out` of >= pack_bound bytes, `out_len` one int64,
        `result` two int32.  `bases`: the pointer array of pack_bases, with
        the members, scratch and bound of a versioned pack:
        fsehip_vpack_compress."""
        p = self._frame_params(chunk_blocks)
        if bases is not None:
            check(self.lib.fsehip_vpack_compress(C.byref(p), members, n, bases, C.c_void_p(scratch.data_ptr()),
                                                 scratch.numel(), C.c_void_p(out.data_ptr()), out.numel(),
                                                 C.c_void_p(out_len.data_ptr()), C.c_void_p(result.data_ptr()),
                                                 self._stream()), "fsehip_vpack_compress")
            return
        check(self.lib.fsehip_pack_compress(C.byref(p), members, n, C.c_void_p(scratch.data_ptr()), scratch.numel(),
                                            C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(out_len.data_ptr()),
                                            C.c_void_p(result.data_ptr()), self._stream()), "fsehip_pack_compress")

    def compress_pack(self, tensors, kinds=None, chunk_blocks: int = 0, bases=None):
        """Compress a list of contiguous device tensors into one pack frame: a
        uint8 device tensor of its exact length.  `kinds`: None (all
        "planes"), one name or one per tensor.  With `bases` (one entry per
        tensor: None, or a contiguous device tensor of the same element size
        and count) the output is a versioned pack, and the kinds default to
        "diff" where a base is given and "planes" where not.  One
        synchronisation, to read the length."""
        t = self.torch
        n, versioned, barr = len(tensors), bases is not None, None
        if versioned:
            kinds, barr = self.pack_bases(tensors, bases, kinds)
        members = self.pack_members(tensors, kinds, versioned)
        bound, need = self.pack_bound(members, n, versioned), self.pack_scratch_bytes(members, n, versioned)
        if not bound or not need:
            raise FseError(-14, "fsehip_pack_bound")
        scratch = t.empty(need, dtype=t.uint8, device=self.device)
        out = t.empty(bound, dtype=t.uint8, device=self.device)
        out_len = t.zeros(1, dtype=t.int64, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self.compress_pack_into(members, n, scratch, out, out_len, result, chunk_blocks, barr)
        return out[: int(out_len.item())]

    @staticmethod
    def pack_info(buf):
        """The head of a pack frame or a versioned pack given as bytes, a
        numpy array or a tensor (its 32 + 16 n + 32 head bytes come to the
        host): a PackHead with `info` (PackInfo), `members` (the PackMember
        array, pointers null), `inner` (the frame's FrameInfo), the lists
        `kinds`, `elem_bytes` and `n_elems`, and `container`, "pack" or
        "vpack"; raises FseError (BAD_FRAME) otherwise."""
        def take(lo, hi):
            if hasattr(buf, "data_ptr"):  # a torch tensor
                return buf[lo:hi].cpu().numpy().tobytes()
            return bytes(memoryview(buf)[lo:hi])

        lib = load()
        info, inner = PackInfo(), FrameInfo()
        a = np.frombuffer(take(0, 32), dtype=np.uint8)
        versioned = lib.fsehip_container_kind(_p(a), len(a)) == KIND_VPACK
        prefix = "fsehip_vpack_" if versioned else "fsehip_pack_"
        check(getattr(lib, prefix + "read_header")(_p(a), len(a), C.byref(info)), prefix + "read_header")
        n = info.n_members
        a = np.frombuffer(take(0, 32 + 16 * n + 32), dtype=np.uint8)
        members = (PackMember * max(n, 1))()
        check(getattr(lib, prefix + "read_members")(_p(a), len(a), members, n, C.byref(info), C.byref(inner)),
              prefix + "read_members")
        return PackHead(info, members, inner, "vpack" if versioned else "pack")

    def _pack_outs(self, head, indices, dtypes, outs):
        """The destinations of the members `indices` after the dtype checks: `outs` or fresh tensors."""
        t = self.torch
        dts = [dtypes] * len(indices) if not isinstance(dtypes, (list, tuple)) else list(dtypes)
        if len(dts) != len(indices):
            raise ValueError(f"{len(dts)} dtypes for {len(indices)} members")
        res, widths = [], {}
        for s, (m, dt) in enumerate(zip(indices, dts)):
            if not 0 <= m < head.info.n_members:
                raise ValueError(f"member {m}: the pack holds {head.info.n_members}")
            w = widths.get(dt) or widths.setdefault(dt, t.empty(0, dtype=dt).element_size())
            if w != head.elem_bytes[m]:
                raise ValueError(f"dtype {dt} has {w}-byte elements, member {m} holds {head.elem_bytes[m]}-byte ones")
            if outs is None:
                res.append(t.empty(head.n_elems[m], dtype=dt, device=self.device))
            else:
                o = outs[s]
                if not o.is_contiguous() or o.dtype != dt or o.numel() != head.n_elems[m]:
                    raise ValueError(f"out {s} must be a contiguous tensor of {head.n_elems[m]} elements of {dt}")
                res.append(o)
        return res

    @staticmethod
    def _pack_point(head, indices, outs):
        """A copy of the head's member array with the members `indices` pointing at `outs`."""
        n = head.info.n_members
        members = (PackMember * max(n, 1))()
        C.memmove(members, head.members, C.sizeof(PackMember) * n)
        for m, o in zip(indices, outs):
            members[m].d_ptr = o.data_ptr() if o.numel() else None
        return members

    def _pack_decode_bases(self, head, indices, bases):
        """The host array of base pointers (one per member of the pack) for a
        decode of the members `indices` of a versioned pack: `bases` a list
        with one entry per index or a dict by member index, None where a
        member has no base; every selected diff member needs one."""
        n = head.info.n_members
        if bases is None:
            given = {}
        elif isinstance(bases, dict):
            given = {int(m): b for m, b in bases.items() if b is not None}
        else:
            bases = list(bases)
            if len(bases) != len(indices):
                raise ValueError(f"{len(bases)} bases for {len(indices)} members")
            given = {m: b for m, b in zip(indices, bases) if b is not None}
        arr = (C.c_void_p * max(n, 1))()
        for m in indices:
            b = given.get(m)
            if b is None:
                if head.kinds[m] == "diff":
                    raise ValueError(f"member {m} is a diff member and decodes against its base: pass bases=")
                continue
            if not hasattr(b, "data_ptr") or not b.is_cuda or not b.is_contiguous():
                raise ValueError(f"base {m}: a versioned pack takes contiguous device tensors")
            if b.element_size() != head.elem_bytes[m] or b.numel() != head.n_elems[m]:
                raise ValueError(f"base {m}: {b.numel()} elements of {b.element_size()} bytes, member {m} holds "
                                 f"{head.n_elems[m]} of {head.elem_bytes[m]}")
            arr[m] = b.data_ptr() if b.numel() else None
        return arr

    def decompress_pack_into(self, buf, head, outs, scratch, block_status, result, chunk_blocks: int = 0,
                             bases=None) -> None:
        """fsehip_pack_decompress, no synchronisation: `head` from pack_info,
        `outs` one contiguous tensor per member (element size and count the
        table's), `scratch` >= pack_scratch_bytes (16-byte aligned),
        `block_status` head.inner.n_blocks int32 or None, `result` two int32.
        A versioned pack (fsehip_vpack_decompress; its scratch is
        pack_scratch_bytes(..., versioned=True)) takes `bases`, one entry per
        member or a dict by index; an out may be its base itself."""
        n = head.info.n_members
        outs = self._pack_outs(head, list(range(n)), [o.dtype for o in outs], outs)
        members = self._pack_point(head, range(n), outs)
        if head.container == "vpack":
            barr = self._pack_decode_bases(head, list(range(n)), bases)
            check(self.lib.fsehip_vpack_decompress(
                C.byref(head.info), members, barr, C.byref(head.inner), chunk_blocks, C.c_void_p(buf.data_ptr()),
                buf.numel(), C.c_void_p(scratch.data_ptr()), scratch.numel(),
                C.c_void_p(block_status.data_ptr()) if block_status is not None else None,
                C.c_void_p(result.data_ptr()), self._stream()), "fsehip_vpack_decompress")
            return
        check(self.lib.fsehip_pack_decompress(
            C.byref(head.info), members, C.byref(head.inner), chunk_blocks, C.c_void_p(buf.data_ptr()), buf.numel(),
            C.c_void_p(scratch.data_ptr()), scratch.numel(),
            C.c_void_p(block_status.data_ptr()) if block_status is not None else None,
            C.c_void_p(result.data_ptr()), self._stream()), "fsehip_pack_decompress")

    def decompress_pack(self, buf, dtypes, chunk_blocks: int = 0, bases=None, outs=None):
        """Decode a pack frame or a versioned pack (a uint8 device tensor)
        into one 1-D tensor per member; `dtypes` is one dtype or one per
        member, each of the member's element size (ValueError otherwise).
        A versioned pack with diff members needs `bases` (one entry per
        member, None where there is none; ValueError without).  `outs`: the
        destinations, fresh tensors by default; outs=bases, or the same
        tensors in both, decodes in place.  Returns (tensors, block_status);
        raises FseError for a frame-level error (BAD_FRAME)."""
        t = self.torch
        head = self.pack_info(buf)
        n, versioned = head.info.n_members, head.container == "vpack"
        if versioned:
            self._pack_decode_bases(head, list(range(n)), bases)  # the argument errors, ahead of any allocation
        outs = self._pack_outs(head, list(range(n)), dtypes, outs)
        scratch = t.empty(self.pack_scratch_bytes(head.members, n, versioned), dtype=t.uint8, device=self.device)
        status = t.zeros(head.inner.n_blocks, dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self.decompress_pack_into(buf, head, outs, scratch, status, result, chunk_blocks, bases)
        check(int(result[0].item()), "pack frame")
        return outs, status

    def decompress_pack_members_into(self, buf, head, indices, outs, scratch, member_status, result,
                                     chunk_blocks: int = 0, bases=None) -> None:
        """fsehip_pack_decompress_members, no synchronisation: `outs` one
        tensor per index, `scratch` >= pack_members_scratch_bytes,
        `member_status` len(indices) int32 or None, `result` two int32.  A
        versioned pack (fsehip_vpack_decompress_members) takes `bases`, a list
        with one entry per index or a dict by member index: the selected diff
        members' are needed."""
        indices = [int(i) for i in indices]
        outs = self._pack_outs(head, indices, [o.dtype for o in outs], outs)
        members = self._pack_point(head, indices, outs)
        sel = (C.c_uint32 * max(len(indices), 1))(*indices)
        if head.container == "vpack":
            barr = self._pack_decode_bases(head, indices, bases)
            check(self.lib.fsehip_vpack_decompress_members(
                C.byref(head.info), members, barr, C.byref(head.inner), chunk_blocks, C.c_void_p(buf.data_ptr()),
                buf.numel(), sel, len(indices), C.c_void_p(scratch.data_ptr()), scratch.numel(),
                C.c_void_p(member_status.data_ptr()) if member_status is not None else None,
                C.c_void_p(result.data_ptr()), self._stream()), "fsehip_vpack_decompress_members")
            return
        check(self.lib.fsehip_pack_decompress_members(
            C.byref(head.info), members, C.byref(head.inner), chunk_blocks, C.c_void_p(buf.data_ptr()), buf.numel(),
            sel, len(indices), C.c_void_p(scratch.data_ptr()), scratch.numel(),
            C.c_void_p(member_status.data_ptr()) if member_status is not None else None,
            C.c_void_p(result.data_ptr()), self._stream()), "fsehip_pack_decompress_members")

    def decompress_pack_members(self, buf, indices, dtypes, chunk_blocks: int = 0, bases=None, outs=None):
        """Decode only the members `indices` of a pack frame or a versioned
        pack (only the blocks they cover are decoded).  `bases`: a list with
        one entry per index or a dict by member index, covering the selected
        diff members of a versioned pack; `outs`: the destinations, fresh
        tensors by default.  Returns (tensors, member_status); raises FseError
        for a frame-level error."""
        t = self.torch
        head = self.pack_info(buf)
        indices = [int(i) for i in indices]
        if len(set(indices)) != len(indices):
            raise ValueError("a member is selected twice")
        versioned = head.container == "vpack"
        outs = self._pack_outs(head, indices, dtypes, outs)
        if versioned:
            self._pack_decode_bases(head, indices, bases)
        need = self.pack_members_scratch_bytes(head.members, head.info.n_members, indices, versioned)
        scratch = t.empty(max(need, 16), dtype=t.uint8, device=self.device)
        status = t.zeros(len(indices), dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self.decompress_pack_members_into(buf, head, indices, outs, scratch, status, result, chunk_blocks, bases)
        check(int(result[0].item()), "pack frame")
        return outs, status

    # ------------------------------------------------------------ the sealed pack
    # (fsehip.h section 2l.)  The member check record -- one CRC-32 per
    # member's content and, for diff members, per base -- in front of an
    # unchanged pack frame or versioned pack.  On decode the bases are verified
    # before the merge may store a byte (one wrong base: nothing is stored, in
    # place or not), the destinations after it.
    def pack_sealed_bound(self, members, n: int, versioned: bool = False) -> int:
        return int(self.lib.fsehip_spack_bound(members, n, int(versioned), self.block_size))

    def pack_sealed_scratch_bytes(self, members, n: int, versioned: bool = False) -> int:
        return int(self.lib.fsehip_spack_scratch_bytes(members, n, int(versioned)))

    def pack_sealed_members_scratch_bytes(self, members, n: int, indices, versioned: bool = False) -> int:
        sel = (C.c_uint32 * max(len(indices), 1))(*indices)
        return int(self.lib.fsehip_spack_members_scratch_bytes(members, n, int(versioned), sel, len(indices)))

    def mcheck_scratch_bytes(self, members, n: int, indices=None, with_bases: bool = False) -> int:
        sel = None if indices is None else (C.c_uint32 * max(len(indices), 1))(*indices)
        return int(self.lib.fsehip_mcheck_scratch_bytes(members, n, sel, 0 if indices is None else len(indices),
                                                        int(with_bases)))

    def mcheck_build(self, tensors, bases=None, kinds=None):
        """The member check record of a list of contiguous device tensors as
        they lie (fsehip_mcheck_build): a uint8 device tensor of 32 + 8 n
        bytes.  With `bases` (as compress_pack) the diff members' base CRCs
        are recorded.  No synchronisation."""
        t = self.torch
        n, versioned, barr = len(tensors), bases is not None, None
        if versioned:
            kinds, barr = self.pack_bases(tensors, bases, kinds)
        members = self.pack_members(tensors, kinds, versioned)
        need = self.mcheck_scratch_bytes(members, n, None, versioned)
        if not need:
            raise FseError(-14, "fsehip_mcheck_scratch_bytes")
        scratch = t.empty(need, dtype=t.uint8, device=self.device)
        record = t.empty(32 + 8 * n, dtype=t.uint8, device=self.device)
        check(self.lib.fsehip_mcheck_build(members, barr, n, C.c_void_p(record.data_ptr()),
                                           C.c_void_p(scratch.data_ptr()), scratch.numel(), self._stream()),
              "fsehip_mcheck_build")
        return record

    def compress_pack_sealed_into(self, members, n: int, scratch, out, out_len, result, chunk_blocks: int = 0,
                                  bases=None, check_bases: bool = True) -> None:
        """fsehip_spack_compress, no synchronisation: as compress_pack_into
        with `scratch` >= pack_sealed_scratch_bytes and `out` >=
        pack_sealed_bound; `bases` (pack_bases' pointer array) makes the inner
        container a versioned pack."""
        p = self._frame_params(chunk_blocks)
        check(self.lib.fsehip_spack_compress(C.byref(p), members, n, bases, int(bool(check_bases)),
                                             C.c_void_p(scratch.data_ptr()), scratch.numel(),
                                             C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(out_len.data_ptr()),
                                             C.c_void_p(result.data_ptr()), self._stream()), "fsehip_spack_compress")

    def compress_pack_sealed(self, tensors, kinds=None, bases=None, check_bases: bool = True, chunk_blocks: int = 0):
        """compress_pack with the member check record in front: a sealed pack,
        a uint8 device tensor of its exact length.  With `bases` the inner
        container is a versioned pack, and with `check_bases` the record also
        holds every diff member's base CRC, so that a decode against another
        base is refused before it stores a byte.  One synchronisation, to read
        the length."""
        t = self.torch
        n, versioned, barr = len(tensors), bases is not None, None
        if versioned:
            kinds, barr = self.pack_bases(tensors, bases, kinds)
        members = self.pack_members(tensors, kinds, versioned)
        bound = self.pack_sealed_bound(members, n, versioned)
        need = self.pack_sealed_scratch_bytes(members, n, versioned)
        if not bound or not need:
            raise FseError(-14, "fsehip_spack_bound")
        scratch = t.empty(need, dtype=t.uint8, device=self.device)
        out = t.empty(bound, dtype=t.uint8, device=self.device)
        out_len = t.zeros(1, dtype=t.int64, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self.compress_pack_sealed_into(members, n, scratch, out, out_len, result, chunk_blocks, barr, check_bases)
        return out[: int(out_len.item())]

    @staticmethod
    def pack_sealed_info(buf):
        """The head of a sealed pack given as bytes, a numpy array or a tensor:
        (record, head) with `record` the McheckInfo of the member check record
        (`record.flags & 1`: base CRCs recorded) and `head` the PackHead of the
        pack behind it, which starts at byte 32 + 8 n; raises FseError
        (BAD_FRAME) otherwise."""
        def take(lo, hi):
            if hasattr(buf, "data_ptr"):  # a torch tensor
                return buf[lo:hi].cpu().numpy().tobytes()
            return bytes(memoryview(buf)[lo:hi])

        lib = load()
        a = np.frombuffer(take(0, 32), dtype=np.uint8)
        rec = McheckInfo()
        check(lib.fsehip_mcheck_read_header(_p(a), len(a), C.byref(rec)), "fsehip_mcheck_read_header")
        off = 32 + 8 * rec.n_members
        a = np.frombuffer(take(0, off + 32), dtype=np.uint8)
        versioned, inner_off = C.c_uint32(0), C.c_uint64(0)
        check(lib.fsehip_spack_read_header(_p(a), len(a), C.byref(rec), C.byref(versioned), C.byref(inner_off)),
              "fsehip_spack_read_header")
        head = BlockCodec.pack_info(np.frombuffer(take(off, off + 32 + 16 * rec.n_members + 32), dtype=np.uint8))
        if (head.container == "vpack") != bool(versioned.value):
            raise FseError(-19, "sealed pack")
        return rec, head

    def _pack_sealed_call(self, buf, rec, head, indices, selected, outs, scratch, status, result, member_check,
                          base_check, check_result, chunk_blocks, bases) -> None:
        versioned = head.container == "vpack"
        outs = self._pack_outs(head, indices, [o.dtype for o in outs], outs)
        members = self._pack_point(head, indices, outs)
        barr = self._pack_decode_bases(head, indices, bases) if versioned else None
        ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
        if selected:
            sel = (C.c_uint32 * max(len(indices), 1))(*indices)
            check(self.lib.fsehip_spack_decompress_members(
                C.byref(rec), C.byref(head.info), int(versioned), members, barr, C.byref(head.inner), chunk_blocks,
                ptr(buf), buf.numel(), sel, len(indices), ptr(scratch), scratch.numel(), ptr(status), ptr(result),
                ptr(member_check), ptr(base_check), ptr(check_result), self._stream()),
                "fsehip_spack_decompress_members")
        else:
            check(self.lib.fsehip_spack_decompress(
                C.byref(rec), C.byref(head.info), int(versioned), members, barr, C.byref(head.inner), chunk_blocks,
                ptr(buf), buf.numel(), ptr(scratch), scratch.numel(), ptr(status), ptr(result), ptr(member_check),
                ptr(base_check), ptr(check_result), self._stream()), "fsehip_spack_decompress")

    def decompress_pack_sealed_into(self, buf, rec, head, outs, scratch, block_status, result, member_check,
                                    base_check, check_result, chunk_blocks: int = 0, bases=None) -> None:
        """fsehip_spack_decompress, no synchronisation: `rec`, `head` from
        pack_sealed_info, `outs`, `block_status`, `result` and `bases` as
        decompress_pack_into, `scratch` >= pack_sealed_scratch_bytes,
        `member_check` / `base_check` one int32 per member or None,
        `check_result` four int32."""
        self._pack_sealed_call(buf, rec, head, list(range(head.info.n_members)), False, outs, scratch, block_status,
                               result, member_check, base_check, check_result, chunk_blocks, bases)

    def decompress_pack_members_sealed_into(self, buf, rec, head, indices, outs, scratch, member_status, result,
                                            member_check, base_check, check_result, chunk_blocks: int = 0,
                                            bases=None) -> None:
        """fsehip_spack_decompress_members, no synchronisation: as
        decompress_pack_members_into with `scratch` >=
        pack_sealed_members_scratch_bytes and the check outputs of
        decompress_pack_sealed_into, one entry per index."""
        self._pack_sealed_call(buf, rec, head, [int(i) for i in indices], True, outs, scratch, member_status, result,
                               member_check, base_check, check_result, chunk_blocks, bases)

    def decompress_pack_sealed(self, buf, dtypes, bases=None, outs=None, chunk_blocks: int = 0,
                               with_result: bool = False):
        """Decode a sealed pack (a uint8 device tensor) as decompress_pack
        does its pack.  The bases of the diff members are verified against the
        record first: if one fails, nothing is stored to any member (with
        outs=bases the old checkpoint is untouched).  Returns (tensors,
        block_status, member_check, base_check): per member FSE_OK or
        CHECKSUM (-21) for the content that lies at its destination after the
        call, and for its base.  Raises FseError for a frame-level error
        (BAD_FRAME) of the pack or of the record.  `with_result`: the four
        int32 of fsehip_spack_decompress's d_check_result as a fifth item."""
        t = self.torch
        rec, head = self.pack_sealed_info(buf)
        n, versioned = head.info.n_members, head.container == "vpack"
        outs = self._pack_outs(head, list(range(n)), dtypes, outs)
        scratch = t.empty(self.pack_sealed_scratch_bytes(head.members, n, versioned), dtype=t.uint8, device=self.device)
        status = t.zeros(head.inner.n_blocks, dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        mcheck = t.zeros(n, dtype=t.int32, device=self.device)
        bcheck = t.zeros(n, dtype=t.int32, device=self.device)
        cres = t.zeros(4, dtype=t.int32, device=self.device)
        self.decompress_pack_sealed_into(buf, rec, head, outs, scratch, status, result, mcheck, bcheck, cres,
                                         chunk_blocks, bases)
        check(int(result[0].item()), "pack frame")
        if int(cres[0].item()) == -19:
            raise FseError(-19, "member check record")
        return (outs, status, mcheck, bcheck, cres) if with_result else (outs, status, mcheck, bcheck)

    def decompress_pack_members_sealed(self, buf, indices, dtypes, bases=None, outs=None, chunk_blocks: int = 0,
                                       with_result: bool = False):
        """Decode only the members `indices` of a sealed pack, as
        decompress_pack_members; whole members are verified, and the gate
        looks at the selected members' bases.  Returns (tensors,
        member_status, member_check, base_check), one entry per index."""
        t = self.torch
        rec, head = self.pack_sealed_info(buf)
        indices = [int(i) for i in indices]
        if len(set(indices)) != len(indices):
            raise ValueError("a member is selected twice")
        versioned = head.container == "vpack"
        outs = self._pack_outs(head, indices, dtypes, outs)
        need = self.pack_sealed_members_scratch_bytes(head.members, head.info.n_members, indices, versioned)
        scratch = t.empty(max(need, 16), dtype=t.uint8, device=self.device)
        status = t.zeros(len(indices), dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        mcheck = t.zeros(len(indices), dtype=t.int32, device=self.device)
        bcheck = t.zeros(len(indices), dtype=t.int32, device=self.device)
        cres = t.zeros(4, dtype=t.int32, device=self.device)
        self.decompress_pack_members_sealed_into(buf, rec, head, indices, outs, scratch, status, result, mcheck, bcheck,
                                                 cres, chunk_blocks, bases)
        check(int(result[0].item()), "pack frame")
        if int(cres[0].item()) == -19:
            raise FseError(-19, "member check record")
        return (outs, status, mcheck, bcheck, cres) if with_result else (outs, status, mcheck, bcheck)

    def block_bytes(self, cb: dict, b: int) -> bytes:
        """Compressed bytes of block b (host copy) -- for parity checks."""
        ln = int(cb["comp_len"][b].item())
        s = b * self.slot_bytes
        return cb["out"][s: s + ln].cpu().numpy().tobytes()


def frame_compress(data, block_size: int = 65536, table_log: int = 0, ckpt_interval: int = 128, nstates: int = 2,
                   device=None) -> bytes:
    """Compress any host buffer (bytes, numpy; empty included) into one frame
    (fsehip.h section 2b) on the GPU; copies through torch."""
    import torch

    codec = BlockCodec(block_size=block_size, table_log=table_log, ckpt_interval=ckpt_interval, device=device,
                       nstates=nstates)
    src = torch.from_numpy(_buf(data).copy()).to(codec.device)
    return codec.compress_frame(src).cpu().numpy().tobytes()


def frame_decompress(data, device=None) -> bytes:
    """Decode a frame held in host memory; raises FseError on a frame-level
    error (BAD_FRAME) or with the first failed block's status."""
    import torch

    codec = BlockCodec(device=device)
    BlockCodec.frame_info(_buf(data))  # not a frame: BAD_FRAME before any device work
    frame = torch.from_numpy(_buf(data).copy()).to(codec.device)
    out, status = codec.decompress_frame(frame)
    st = status.cpu().numpy()
    if st.any():
        b = int(np.flatnonzero(st)[0])
        raise FseError(int(st[b]), f"frame block {b}")
    return out.cpu().numpy().tobytes()


def frame_decompress_range(data, offset: int, length: int, device=None) -> bytes:
    """Raw bytes [offset, offset + length) of a frame held in host memory;
    raises FseError as BlockCodec.decompress_frame_range.  The whole frame is
    uploaded: sending only the header, the directory and the records the
    range needs is out of scope here."""
    import torch

    codec = BlockCodec(device=device)
    BlockCodec.frame_info(_buf(data))  # not a frame: BAD_FRAME before any device work
    frame = torch.from_numpy(_buf(data).copy()).to(codec.device)
    return codec.decompress_frame_range(frame, offset, length).cpu().numpy().tobytes()


# the integer view a host array of each item size travels as
_INT_VIEW = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}


def _host_base(a: np.ndarray, base) -> np.ndarray:
    """A diff frame's base on the host: an array of a's dtype and element count (ValueError otherwise)."""
    if base is None:
        raise ValueError("the diff frame needs its base array")
    b = np.ascontiguousarray(base)
    if b.dtype != a.dtype or b.size != a.size:
        raise ValueError(f"base has {b.size} items of {b.dtype}, the array {a.size} of {a.dtype}")
    return b.reshape(-1).view(_INT_VIEW[b.dtype.itemsize])


def _elem_compress(kind: str, data, block_size: int, table_log: int, ckpt_interval: int, nstates: int, device,
                   base=None) -> bytes:
    """Compress a numpy array of one of the kind's item sizes into one frame
    of the kind on the GPU; copies through torch.  The element width is
    stored, the dtype and the shape are not."""
    import torch

    a = np.ascontiguousarray(data)
    if a.dtype.itemsize not in _ELEM[kind].widths:
        raise ValueError(f"item size {a.dtype.itemsize}: the {_ELEM[kind].label} frame takes {_ELEM[kind].takes} bytes")
    codec = BlockCodec(block_size=block_size, table_log=table_log, ckpt_interval=ckpt_interval, device=device,
                       nstates=nstates)
    src = torch.from_numpy(a.reshape(-1).view(_INT_VIEW[a.dtype.itemsize]).copy()).to(codec.device)
    dbase = torch.from_numpy(_host_base(a, base).copy()).to(codec.device) if _ELEM[kind].based else None
    return codec._elem_compress(kind, src, 0, dbase).cpu().numpy().tobytes()


def _elem_decompress(kind: str, data, dtype, device, base=None) -> np.ndarray:
    """Decode a frame of the kind held in host memory into a 1-D numpy array
    of `dtype` (its item size must be the frame's element width); raises
    FseError on a frame-level error or with the first failed block's status."""
    import torch

    dt, label = np.dtype(dtype), _ELEM[kind].label
    codec = BlockCodec(device=device)
    info, _ = BlockCodec._elem_info(kind, _buf(data))  # not a frame of the kind: BAD_FRAME before any device work
    if dt.itemsize != info.elem_bytes:
        raise ValueError(f"dtype {dt} has {dt.itemsize}-byte items, the {label} frame holds {info.elem_bytes}-byte ones")
    buf = torch.from_numpy(_buf(data).copy()).to(codec.device)
    dbase = None
    if _ELEM[kind].based:
        dbase = torch.from_numpy(_host_base(np.empty(info.n_elems, dtype=dt), base).copy()).to(codec.device)
    out, status = codec._elem_decompress(kind, buf, getattr(torch, np.dtype(_INT_VIEW[info.elem_bytes]).name), 0,
                                         dbase)
    st = status.cpu().numpy()
    if st.any():
        b = int(np.flatnonzero(st)[0])
        raise FseError(int(st[b]), f"{label} frame block {b}")
    return out.cpu().numpy().view(dt)


def planes_compress(data, block_size: int = 65536, table_log: int = 0, ckpt_interval: int = 128, nstates: int = 2,
                    device=None) -> bytes:
    """`_elem_compress` of a numpy array of item size 2, 4 or 8 into one plane frame (fsehip.h section 2d)."""
    return _elem_compress("planes", data, block_size, table_log, ckpt_interval, nstates, device)


def planes_decompress(data, dtype, device=None) -> np.ndarray:
    """`_elem_decompress` of a plane frame held in host memory."""
    return _elem_decompress("planes", data, dtype, device)


def delta_compress(data, block_size: int = 65536, table_log: int = 0, ckpt_interval: int = 128, nstates: int = 2,
                   device=None) -> bytes:
    """`_elem_compress` of a numpy array of item size 1, 2, 4 or 8 into one delta frame (fsehip.h section 2e)."""
    return _elem_compress("delta", data, block_size, table_log, ckpt_interval, nstates, device)


def delta_decompress(data, dtype, device=None) -> np.ndarray:
    """`_elem_decompress` of a delta frame held in host memory."""
    return _elem_decompress("delta", data, dtype, device)


def diff_compress(data, base, block_size: int = 65536, table_log: int = 0, ckpt_interval: int = 128, nstates: int = 2,
                  device=None) -> bytes:
    """`_elem_compress` of a numpy array of item size 1, 2, 4 or 8 against a
    base array of its dtype and size into one diff frame (fsehip.h section 2h)."""
    return _elem_compress("diff", data, block_size, table_log, ckpt_interval, nstates, device, base)


def diff_decompress(data, base, device=None) -> np.ndarray:
    """`_elem_decompress` of a diff frame held in host memory against `base`,
    a numpy array of the frame's element count; the result has its dtype.
    The frame does not identify its base: see BlockCodec.decompress_diff."""
    if base is None:
        raise ValueError("the diff frame needs its base array")
    return _elem_decompress("diff", data, np.asarray(base).dtype, device, base)


# ---------------------------------------------------------------- the size estimate and the automatic choice
def pack_info(buf):
    """`BlockCodec.pack_info`: the head of a pack frame (fsehip.h section 2j)."""
    return BlockCodec.pack_info(buf)


def _pack_host_tensors(arrays, what, device, optional=False):
    """The arrays of a host pack call as flat integer device tensors (None stays None where `optional`)."""
    import torch

    tensors = []
    for m, data in enumerate(arrays):
        if data is None and optional:
            tensors.append(None)
            continue
        a = np.ascontiguousarray(data)
        if a.dtype.itemsize not in _INT_VIEW:
            raise ValueError(f"{what} {m}: item size {a.dtype.itemsize}: a pack takes 1, 2, 4 or 8 bytes")
        tensors.append(torch.from_numpy(a.reshape(-1).view(_INT_VIEW[a.dtype.itemsize]).copy()).to(device))
    return tensors


def pack_compress(arrays, kinds=None, block_size: int = 65536, table_log: int = 0, ckpt_interval: int = 128,
                  nstates: int = 2, device=None, bases=None) -> bytes:
    """Compress a list of numpy arrays of item size 1, 2, 4 or 8 into one pack
    frame on the GPU; copies through torch.  `kinds`: None (all "planes"), one
    name or one per array.  With `bases` (one entry per array: None or an
    array of the same item size and count) the output is a versioned pack, as
    BlockCodec.compress_pack.  The element widths are stored, dtypes and
    shapes are not."""
    codec = BlockCodec(block_size=block_size, table_log=table_log, ckpt_interval=ckpt_interval, device=device,
                       nstates=nstates)
    tensors = _pack_host_tensors(arrays, "member", codec.device)
    if bases is not None:
        bases = _pack_host_tensors(bases, "base", codec.device, optional=True)
    return codec.compress_pack(tensors, kinds, bases=bases).cpu().numpy().tobytes()


def pack_decompress(blob, dtypes, device=None, bases=None) -> list:
    """Decode a pack frame or a versioned pack held in host memory into one
    1-D numpy array per member; `dtypes` is one dtype or one per member (each
    of the member's item size); `bases`: one entry per member, None or the
    array a diff member was coded against; raises FseError on a frame-level
    error or with the first failed block's status."""
    import torch

    head = BlockCodec.pack_info(_buf(blob))  # not a pack: BAD_FRAME before any device work
    n = head.info.n_members
    dts = [np.dtype(d) for d in (dtypes if isinstance(dtypes, (list, tuple)) else [dtypes] * n)]
    if len(dts) != n:
        raise ValueError(f"{len(dts)} dtypes for {n} members")
    for m, dt in enumerate(dts):
        if dt.itemsize != head.elem_bytes[m]:
            raise ValueError(f"dtype {dt} has {dt.itemsize}-byte items, member {m} holds {head.elem_bytes[m]}-byte ones")
    codec = BlockCodec(device=device)
    buf = torch.from_numpy(_buf(blob).copy()).to(codec.device)
    if bases is not None:
        bases = _pack_host_tensors(bases, "base", codec.device, optional=True)
    outs, status = codec.decompress_pack(buf, [getattr(torch, np.dtype(_INT_VIEW[w]).name) for w in head.elem_bytes],
                                         bases=bases)
    st = status.cpu().numpy()
    if st.any():
        b = int(np.flatnonzero(st)[0])
        raise FseError(int(st[b]), f"pack frame block {b}")
    return [o.cpu().numpy().view(dt) for o, dt in zip(outs, dts)]


def pack_sealed_info(buf):
    """`BlockCodec.pack_sealed_info`: the record and the head of a sealed pack (fsehip.h section 2l)."""
    return BlockCodec.pack_sealed_info(buf)


def pack_sealed_compress(arrays, kinds=None, bases=None, check_bases: bool = True, block_size: int = 65536,
                         table_log: int = 0, ckpt_interval: int = 128, nstates: int = 2, device=None) -> bytes:
    """pack_compress with the member check record in front (a sealed pack,
    fsehip.h section 2l); with `bases` and `check_bases` the record holds the
    diff members' base CRCs as well."""
    codec = BlockCodec(block_size=block_size, table_log=table_log, ckpt_interval=ckpt_interval, device=device,
                       nstates=nstates)
    tensors = _pack_host_tensors(arrays, "member", codec.device)
    if bases is not None:
        bases = _pack_host_tensors(bases, "base", codec.device, optional=True)
    return codec.compress_pack_sealed(tensors, kinds, bases=bases, check_bases=check_bases).cpu().numpy().tobytes()


def pack_sealed_decompress(blob, dtypes, bases=None, device=None) -> list:
    """Decode a sealed pack held in host memory as pack_decompress does a
    pack, and verify it: raises FseError("CHECKSUM") naming the members whose
    base does not match the record (nothing was decoded then) or, failing
    that, the members whose content does not; BAD_FRAME for a damaged head;
    the first failed block's status otherwise."""
    import torch

    rec, head = BlockCodec.pack_sealed_info(_buf(blob))  # not a sealed pack: BAD_FRAME before any device work
    n = head.info.n_members
    dts = [np.dtype(d) for d in (dtypes if isinstance(dtypes, (list, tuple)) else [dtypes] * n)]
    if len(dts) != n:
        raise ValueError(f"{len(dts)} dtypes for {n} members")
    for m, dt in enumerate(dts):
        if dt.itemsize != head.elem_bytes[m]:
            raise ValueError(f"dtype {dt} has {dt.itemsize}-byte items, member {m} holds {head.elem_bytes[m]}-byte ones")
    codec = BlockCodec(device=device)
    buf = torch.from_numpy(_buf(blob).copy()).to(codec.device)
    if bases is not None:
        bases = _pack_host_tensors(bases, "base", codec.device, optional=True)
    outs, status, mcheck, bcheck = codec.decompress_pack_sealed(
        buf, [getattr(torch, np.dtype(_INT_VIEW[w]).name) for w in head.elem_bytes], bases=bases)
    bad_base = np.flatnonzero(bcheck.cpu().numpy())
    if bad_base.size:
        raise FseError(-21, f"sealed pack: base of member(s) {bad_base.tolist()} differs from the recorded base; "
                            "nothing was decoded")
    st = status.cpu().numpy()
    if st.any():
        b = int(np.flatnonzero(st)[0])
        raise FseError(int(st[b]), f"pack frame block {b}")
    bad = np.flatnonzero(mcheck.cpu().numpy())
    if bad.size:
        raise FseError(-21, f"sealed pack: content of member(s) {bad.tolist()}")
    return [o.cpu().numpy().view(dt) for o, dt in zip(outs, dts)]


def log2q8(c: int) -> int:
    """`fsehip_log2q8`: the estimate's 256 * log2(c) for 1 <= c <= 32768 (host, no device)."""
    if not 1 <= c <= 32768:
        raise ValueError(f"log2q8({c}): 1..32768")
    return int(load().fsehip_log2q8(c))


def estimate_choose(est):
    """`fsehip_estimate_choose`: the kind name of the smallest estimate of a
    dict kind name -> bytes (BlockCodec.estimate's) or a 3-sequence indexed by
    kind with EST_NONE for a missing one; ties go to frame, then planes, then
    delta.  A dict with "diff" or a 5-sequence (entry 3 takes no part) goes to
    `fsehip_estimate_choose_base`: the diff frame is last in a tie.
    ValueError when there is nothing to choose from."""
    if isinstance(est, dict) and "diff" in est:
        est = [est.get(name, EST_NONE) if name else EST_NONE for name in _BASE_KINDS]
    if not isinstance(est, dict) and len(est) == 5:
        arr = (C.c_uint64 * 5)(*[int(v) for v in est])
        k = load().fsehip_estimate_choose_base(C.byref(arr))
        if k < 0:
            raise ValueError("no estimate to choose from")
        return _BASE_KINDS[k]
    if isinstance(est, dict):
        est = [est.get(name, EST_NONE) for name in KINDS]
    arr = (C.c_uint64 * 3)(*[int(v) for v in est])
    k = load().fsehip_estimate_choose(C.byref(arr))
    if k < 0:
        raise ValueError("no estimate to choose from")
    return KINDS[k]


def container_kind(buf) -> str:
    """`fsehip_container_kind`: "frame", "planes", "delta", "sealed", "diff", "pack", "vpack" or "spack" from
    the magic of a container given as bytes, a numpy array or a tensor (its
    first 4 bytes come to the host); raises FseError (BAD_FRAME) for anything
    else."""
    if hasattr(buf, "data_ptr"):  # a torch tensor
        head = buf[:4].cpu().numpy().tobytes()
    else:
        head = bytes(memoryview(buf)[:4])
    a = np.frombuffer(head, dtype=np.uint8)
    k = load().fsehip_container_kind(_p(a), len(a))
    if k < 0:
        raise FseError(k, "fsehip_container_kind")
    if k == KIND_VPACK:
        return "vpack"
    if k == KIND_SPACK:
        return "spack"
    return "sealed" if k == KIND_SEALED else "diff" if k == KIND_DIFF else "pack" if k == KIND_PACK else KINDS[k]


def auto_compress(data, kinds=None, block_size: int = 65536, table_log: int = 0, ckpt_interval: int = 128,
                  nstates: int = 2, device=None, base=None):
    """Compress a numpy array of item size 1, 2, 4 or 8 into whichever of the
    frame, the plane frame and the delta frame -- and, with `base`, an array
    of its dtype and size, the diff frame against it -- the estimate finds
    smallest (BlockCodec.compress_auto) on the GPU; copies through torch.
    Returns (bytes, kind name)."""
    import torch

    a = np.ascontiguousarray(data)
    if a.dtype.itemsize not in _INT_VIEW:
        raise ValueError(f"item size {a.dtype.itemsize}: the containers take 1, 2, 4 or 8 bytes")
    codec = BlockCodec(block_size=block_size, table_log=table_log, ckpt_interval=ckpt_interval, device=device,
                       nstates=nstates)
    src = torch.from_numpy(a.reshape(-1).view(_INT_VIEW[a.dtype.itemsize]).copy()).to(codec.device)
    dbase = None if base is None else torch.from_numpy(_host_base(a, base).copy()).to(codec.device)
    buf, kind = codec.compress_auto(src, kinds, base=dbase)
    return buf.cpu().numpy().tobytes(), kind


def auto_decompress(blob, dtype, device=None, base=None) -> np.ndarray:
    """Decode what auto_compress returned -- or a diff frame, with its base
    array as `base` (ValueError without) -- by its magic, into a 1-D numpy
    array of `dtype`; raises FseError as frame_decompress / planes_decompress
    / delta_decompress / diff_decompress."""
    kind = container_kind(_buf(blob))
    if kind == "diff" and base is None:
        raise ValueError("a diff frame decodes against its base: pass base=")
    if kind in _ELEM:
        return _elem_decompress(kind, blob, dtype, device, base if kind == "diff" else None)
    if kind in ("pack", "vpack"):
        raise ValueError("a pack frame holds many tensors and goes to pack_decompress")
    if kind != "frame":
        raise ValueError("a sealed buffer goes to sealed_decompress")
    return np.frombuffer(frame_decompress(blob, device), dtype=np.dtype(dtype))


# ---------------------------------------------------------------- sealed buffers
def crc32(data, crc: int = 0) -> int:
    """`fsehip_crc32`: zlib.crc32(data, crc), computed by the library on the host (no device)."""
    a = _buf(data)
    return int(load().fsehip_crc32(crc & 0xFFFFFFFF, _p(a) if len(a) else None, len(a))) if len(a) else crc & 0xFFFFFFFF


def crc32_combine(crc1: int, crc2: int, len2: int) -> int:
    """`fsehip_crc32_combine`: the CRC-32 of A || B from crc32(A), crc32(B) and len(B) (no device)."""
    return int(load().fsehip_crc32_combine(crc1 & 0xFFFFFFFF, crc2 & 0xFFFFFFFF, len2))


def sealed_compress(data, kind: str = "frame", check_block: int = 65536, block_size: int = 65536, table_log: int = 0,
                    ckpt_interval: int = 128, nstates: int = 2, device=None, base=None) -> bytes:
    """Compress a host buffer into one sealed buffer (fsehip.h section 2f) on
    the GPU: bytes or any numpy array for kind 'frame', a numpy array of item
    size 2, 4 or 8 for 'planes' and of 1, 2, 4 or 8 for 'delta' and for
    'diff', which codes it against `base`, an array of its dtype and size.
    kind 'auto' (a numpy array of item size 1, 2, 4 or 8, or bytes) seals the
    kind the estimate finds smallest, the diff frame among them when `base`
    is given (BlockCodec.compress_sealed)."""
    import torch

    codec = BlockCodec(block_size=block_size, table_log=table_log, ckpt_interval=ckpt_interval, device=device,
                       nstates=nstates)
    if kind == "frame":
        a = _buf(data) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    else:
        a = np.ascontiguousarray(data) if isinstance(data, np.ndarray) or kind != "auto" else _buf(data)
        if a.dtype.itemsize not in _INT_VIEW:
            raise ValueError(f"item size {a.dtype.itemsize}: 1, 2, 4 or 8 bytes")
        if kind == "diff" or (kind == "auto" and base is not None):
            base = torch.from_numpy(_host_base(a, base).copy()).to(codec.device)
        a = a.reshape(-1).view(_INT_VIEW[a.dtype.itemsize])
    src = torch.from_numpy(a.copy()).to(codec.device)
    return codec.compress_sealed(src, kind, check_block, base=base).cpu().numpy().tobytes()


def sealed_decompress(blob, dtype=None, device=None, base=None):
    """Decode a sealed buffer held in host memory: bytes for a sealed frame, a
    1-D numpy array of `dtype` (default: the integer of the element width) for
    a plane, delta or diff frame; the last needs `base`, an array of the
    frame's element count and width, and a wrong one raises CHECKSUM.  Raises
    FseError on a buffer-level error
    (BAD_FRAME), with the first failed block's status, and with CHECKSUM when
    a check block or the whole content's CRC-32 fails."""
    import torch

    codec = BlockCodec(device=device)
    info, kind, off = BlockCodec.sealed_info(_buf(blob))  # not a sealed buffer: BAD_FRAME before any device work
    buf = torch.from_numpy(_buf(blob).copy()).to(codec.device)
    dt = None if dtype is None else np.dtype(dtype)
    dbase = None
    if kind == "diff":
        if base is None:
            raise ValueError("a sealed diff buffer needs base=")
        b = np.ascontiguousarray(base).reshape(-1)
        if b.dtype.itemsize not in _INT_VIEW:
            raise ValueError(f"item size {b.dtype.itemsize}: 1, 2, 4 or 8 bytes")
        dbase = torch.from_numpy(b.view(_INT_VIEW[b.dtype.itemsize]).copy()).to(codec.device)
    out, status, check_status, result = codec.decompress_sealed(buf, None, with_result=True, base=dbase)
    if dt is not None and dt.itemsize != out.element_size():
        raise ValueError(f"dtype {dt} has {dt.itemsize}-byte items, the sealed buffer holds {out.element_size()}-byte ones")
    st = status.cpu().numpy()
    if st.any():
        b = int(np.flatnonzero(st)[0])
        raise FseError(int(st[b]), f"sealed {kind} block {b}")
    cs, res = check_status.cpu().numpy(), result.cpu().numpy()
    if cs.any():
        b = int(np.flatnonzero(cs)[0])
        raise FseError(int(cs[b]), f"sealed {kind} check block {b}")
    check(int(res[0]), f"sealed {kind} content")
    host = out.cpu().numpy()
    if kind == "frame" and dt is None:
        return host.tobytes()
    return host.view(dt) if dt is not None else host


# ---------------------------------------------------------------- shared-table coding
def norm_histogram_try_from(table) -> NormHistogram:
    """`NormHistogram::try_from([i32; 256])` (histogram.rs:508-536): the sum of
    |x| must be a power of two; table_len = 1 + the last non-zero index.  Host only."""
    a = np.ascontiguousarray(table, dtype=np.int32)
    if a.shape != (256,):
        raise ValueError("a table of 256 counts")
    nh = NormHistogram()
    check(load().norm_histogram_try_from(_p(a), C.byref(nh)), "norm_histogram_try_from")
    return nh


class SharedTable:
    """One caller's table on the device and many small messages coded against
    it, with no header in front (fsehip.h section 2c): the crate's
    `EncodeTable::new(&nh)` / `DecodeTable::new(&nh)` with an `Encoder` /
    `Decoder` per message (fse.rs:86-386).  `status` is the name of the build's
    status; a failed build raises unless check_build=False (every message coded
    with such a table is BAD_TABLE)."""

    def __init__(self, nh: NormHistogram, device=None, check_build: bool = True):
        import torch

        from ._lib import STATUS

        self.lib = load()
        self.device = torch.device(device or "cuda")
        self.table_log = int(nh.log2)
        d_nh = torch.from_numpy(np.frombuffer(bytes(nh), dtype=np.uint8).copy()).to(self.device)
        self.image = torch.zeros(int(self.lib.fsehip_shared_table_bytes()), dtype=torch.uint8, device=self.device)
        st = torch.zeros(1, dtype=torch.int32, device=self.device)
        check(self.lib.fsehip_shared_table_build(C.c_void_p(d_nh.data_ptr()), C.c_void_p(self.image.data_ptr()),
                                                 C.c_void_p(st.data_ptr()), self._stream()),
              "fsehip_shared_table_build")
        rc = int(st.cpu()[0])
        self.status = STATUS.get(rc, str(rc))
        if check_build and rc != 0:
            raise FseError(rc, "fsehip_shared_table_build")

    @classmethod
    def train(cls, samples, table_log: int = 11, floor: int = 1, device=None) -> "SharedTable":
        """A table for messages like `samples`: their histogram plus `floor` on
        all 256 symbols (with floor >= 1 every byte has a slot), through
        `Histogram::normalize(table_log)`."""
        h = histogram_new(np.concatenate([_buf(x) for x in samples]))
        for s in range(256):
            h.counts[s] += floor
        h.size += 256 * floor
        if floor:
            h.table_len = 256
        return cls(normalize(h, table_log), device=device)

    def _stream(self):
        import torch

        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _upload(self, bufs, caps):
        """Inputs back to back at 16-byte aligned offsets, output regions 64
        bytes apart and filled with 0xA5, as compress_streams lays them out."""
        import torch

        from ._lib import StreamDesc

        n, dev = len(bufs), self.device
        desc = (StreamDesc * max(n, 1))()
        so = oo = 0
        for i, b in enumerate(bufs):
            desc[i] = StreamDesc(so, oo, len(b), caps[i])
            so += (len(b) + 15) // 16 * 16
            oo += (caps[i] + 15) // 16 * 16 + 64
        host = np.zeros(max(so, 16), dtype=np.uint8)
        for i, b in enumerate(bufs):
            host[desc[i].src_off: desc[i].src_off + len(b)] = b
        d_in = torch.from_numpy(host).to(dev)
        d_desc = torch.from_numpy(np.frombuffer(bytes(desc), dtype=np.uint8).copy()).to(dev)
        out = torch.full((max(oo, 16),), 0xA5, dtype=torch.uint8, device=dev)
        lens = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        return desc, d_in, d_desc, out, lens, status

    def compress(self, buffers, nstates: int = 2, out_caps=None, raw: bool = False):
        """`fsehip_compress_shared`: per message (payload bytes, payload bits)
        or the name of its status.  out_caps[i] bytes per output region
        (default `fsehip_shared_out_bytes`).  raw=True: (statuses, lengths,
        payload bits, out bytes as numpy, descriptors) for bounds checks."""
        import torch

        from ._lib import STATUS

        bufs = [_buf(x) for x in buffers]
        n = len(bufs)
        caps = ([int(self.lib.fsehip_shared_out_bytes(len(b), self.table_log)) for b in bufs]
                if out_caps is None else list(out_caps))
        desc, d_src, d_desc, out, comp_len, status = self._upload(bufs, caps)
        bits = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        check(self.lib.fsehip_compress_shared(nstates, p(self.image), p(d_src), p(d_desc), n, p(out), p(comp_len),
                                              p(bits), p(status), self._stream()), "fsehip_compress_shared")
        torch.cuda.synchronize(self.device)
        ho, cl, pb, st = out.cpu().numpy(), comp_len.cpu().numpy()[:n], bits.cpu().numpy()[:n], status.cpu().numpy()[:n]
        if raw:
            return st, cl, pb, ho, [(d.src_off, d.out_off, d.src_len, d.out_cap) for d in desc[:n]]
        return [(ho[desc[i].out_off: desc[i].out_off + int(cl[i])].tobytes(), int(pb[i])) if st[i] == 0 else
                STATUS.get(int(st[i]), str(int(st[i]))) for i in range(n)]

    def decompress(self, payloads, raw_lens=None, nstates: int = 2, out_cap=None, raw: bool = False):
        """`fsehip_decompress_shared`: per payload its bytes or the name of its
        status.  raw_lens: the messages' lengths (the payload must end with
        exactly that many bytes), or None: each ends where the crate's decoder
        stops.  out_cap: bytes per output region, one number or a list
        (default: the raw length, or 65,536 without lengths).  raw=True:
        (statuses, lengths, out bytes as numpy, descriptors)."""
        import torch

        from ._lib import STATUS

        bufs = [_buf(x) for x in payloads]
        n = len(bufs)
        if out_cap is None:
            caps = [int(x) for x in raw_lens] if raw_lens is not None else [65536] * n
        else:
            caps = [int(out_cap)] * n if np.isscalar(out_cap) else [int(x) for x in out_cap]
        desc, d_in, d_desc, out, out_len, status = self._upload(bufs, caps)
        d_raw = None
        if raw_lens is not None:
            d_raw = torch.from_numpy(np.array(list(raw_lens) or [0], dtype=np.uint32).view(np.int32)).to(self.device)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        check(self.lib.fsehip_decompress_shared(nstates, p(self.image), p(d_in), p(d_desc), n, p(out),
                                                p(d_raw) if d_raw is not None else None, p(out_len), p(status),
                                                self._stream()), "fsehip_decompress_shared")
        torch.cuda.synchronize(self.device)
        ho, ol, st = out.cpu().numpy(), out_len.cpu().numpy()[:n], status.cpu().numpy()[:n]
        if raw:
            return st, ol, ho, [(d.src_off, d.out_off, d.src_len, d.out_cap) for d in desc[:n]]
        return [ho[desc[i].out_off: desc[i].out_off + int(ol[i])].tobytes() if st[i] == 0 else
                STATUS.get(int(st[i]), str(int(st[i]))) for i in range(n)]


__all__ = ["BITS_ADVANCE", "BITS_PEEK", "BITS_READ", "BitStackReader", "BitStackWriter", "BitStreamReader", "BlockCodec", "DecodeTable", "EncodeTable", "FseError",
           "Histogram", "NormHistogram", "bitstack_read", "bitstack_write", "bitstream_read", "compress", "compress2",
           "compress2_log", "compress2_many", "compress_nh", "compress_streams", "decode_table_new", "decompress", "decompress2", "decompress2_many",
           "decompress_streams",
           "encode_table_new", "frame_compress", "frame_decompress", "frame_decompress_range",
           "histogram_count", "histogram_new", "norm_histogram_new", "norm_histogram_read", "norm_histogram_write",
           "normalize", "normalize_optimal", "SharedTable", "norm_histogram_try_from",
           "planes_compress", "planes_decompress", "delta_compress", "delta_decompress", "diff_compress",
           "diff_decompress",
           "sealed_compress", "sealed_decompress", "crc32", "crc32_combine", "CheckInfo",
           "auto_compress", "auto_decompress", "container_kind", "estimate_choose", "log2q8",
           "pack_compress", "pack_decompress", "pack_info", "PackHead",
           "pack_sealed_compress", "pack_sealed_decompress", "pack_sealed_info", "McheckInfo", "MCHECK_BASES"]
