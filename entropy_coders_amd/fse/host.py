"""Reference-shaped calls (host bytes in, bytes out; lib.rs:146-248,
histogram.rs:18-66), their many-buffer forms and the building blocks as
plain data: fsehip.h sections 1a and 1b, fse_capi_host.cpp."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .._lib import STATUS, DecodeTable, EncodeTable, FseError, Histogram, NormHistogram, check, load
from ._helpers import _buf, _lay_out_streams, _out, _p, _ptr

__all__ = ["DecodeTable", "EncodeTable", "FseError", "Histogram", "NormHistogram", "compress", "compress2",
           "compress2_log", "compress2_many", "compress_nh", "compress_streams", "decode_table_new", "decompress",
           "decompress2", "decompress2_many", "decompress_streams", "encode_table_new", "histogram_count",
           "histogram_new", "norm_histogram_new", "norm_histogram_read", "norm_histogram_write", "normalize",
           "normalize_optimal"]


def compress2(src) -> tuple[bytes, int]:
    """`fse_compress2(src, &mut dst) -> usize` (lib.rs:146): (bytes, payload bits)."""
    a = _buf(src)
    lib = load()
    cap = int(lib.fsehip_slot_bytes(max(len(a), 16), 12))
    dst = _out(cap)
    n, bits = C.c_size_t(0), C.c_uint64(0)
    check(lib.fse_compress2(_p(a), len(a), _p(dst), cap, C.byref(n), C.byref(bits)), "fse_compress2")
    return dst[: n.value].tobytes(), bits.value


def compress2_log(src, table_log: int) -> tuple[bytes, int]:
    """`Histogram::new(src).normalize(L)` + fse_compress2 body (histogram.rs:95)."""
    a = _buf(src)
    lib = load()
    cap = int(lib.fsehip_slot_bytes(max(len(a), 16), 12))
    dst = _out(cap)
    n, bits = C.c_size_t(0), C.c_uint64(0)
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
    n, bits = C.c_size_t(0), C.c_uint64(0)
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
    check(load().fsehip_decompress_streams(nstates, max_table_log, _ptr(d_in), stride, _ptr(lens), len(streams),
                                           _ptr(out), out_stride, _ptr(out_len), _ptr(status),
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

    lib = load()
    dev = torch.device(device or "cuda")
    bufs = [_buf(x) for x in buffers]
    n = len(bufs)
    lmax = max_table_log or (max(11, min(table_log, 15)) if table_log else 11)
    caps = [int(lib.fsehip_stream_out_bytes(len(b), lmax)) for b in bufs] if out_caps is None else list(out_caps)
    desc, d_src, d_desc, out = _lay_out_streams(torch, bufs, caps, dev)
    comp_len = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    bits = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    check(lib.fsehip_compress_streams(nstates, table_log, max_table_log, _ptr(d_src), _ptr(d_desc), n, _ptr(out),
                                      _ptr(comp_len), _ptr(bits), _ptr(status),
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
    n, bits = C.c_size_t(0), C.c_uint64(0)
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
    n, bits = C.c_size_t(0), C.c_uint64(0)
    nh = NormHistogram()
    check(lib.fse_compress_nh(_p(a), len(a), _p(dst), cap, C.byref(n), C.byref(bits), C.byref(nh)), "fse_compress_nh")
    return dst[: n.value].tobytes(), bits.value, nh
