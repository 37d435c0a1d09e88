"""The element frames (fsehip.h sections 2d, 2e and 2h, fse_capi_elem.cpp):
one container under three names.  The plane frame puts byte k of every
element into plane k and codes the planes by one frame.  The delta frame
first takes the zigzag differences of neighbouring elements, with a restart
every 4,096: for integer tensors that grow (sorted ids, offsets,
timestamps); any dtype of 1, 2, 4 or 8 bytes round-trips, floats gain
nothing.  The container stores the element width; dtype and shape stay with
the caller.  The diff frame takes the zigzag differences against a base
tensor of the same dtype and element count that the receiver already holds,
and needs that base to decode; the container does not identify it (a sealed
buffer's checksums tell a wrong one)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .._lib import DeltaInfo, DiffInfo, FrameInfo, PlanesInfo, PlanesRange, check, load
from ._helpers import _INT_VIEW, _back_to_back, _buf, _head, _p, _ptr, _raise_first_failed, _upload
from .core import _CodecCore

__all__ = ["planes_compress", "planes_decompress", "delta_compress", "delta_decompress", "diff_compress",
           "diff_decompress"]


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


class _ElemCodec(_CodecCore):
    # The `_elem_*` methods take the kind, "planes", "delta" or "diff" (a row
    # of _ELEM), and `base` for "diff" alone; the public names forward.
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
        a = _head(buf, 48)
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
                        out.numel() * out.element_size(), _ptr(block_status), C.c_void_p(result.data_ptr()),
                        self._stream())

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
                        _ptr(range_status), C.c_void_p(result.data_ptr()), self._stream())

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
        packed, at = _back_to_back(ranges)
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
        return _ElemCodec._elem_info("planes", buf)

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
        return _ElemCodec._elem_info("delta", buf)

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
        return _ElemCodec._elem_info("diff", buf)

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
    codec = _ElemCodec(block_size, table_log, ckpt_interval, device, nstates)
    src = _upload(torch, a.reshape(-1).view(_INT_VIEW[a.dtype.itemsize]), codec.device)
    dbase = _upload(torch, _host_base(a, base), codec.device) if _ELEM[kind].based else None
    return codec._elem_compress(kind, src, 0, dbase).cpu().numpy().tobytes()


def _elem_decompress(kind: str, data, dtype, device, base=None) -> np.ndarray:
    """Decode a frame of the kind held in host memory into a 1-D numpy array
    of `dtype` (its item size must be the frame's element width); raises
    FseError on a frame-level error or with the first failed block's status."""
    import torch

    dt, label = np.dtype(dtype), _ELEM[kind].label
    codec = _ElemCodec(device=device)
    info, _ = codec._elem_info(kind, _buf(data))  # not a frame of the kind: BAD_FRAME before any device work
    if dt.itemsize != info.elem_bytes:
        raise ValueError(f"dtype {dt} has {dt.itemsize}-byte items, the {label} frame holds {info.elem_bytes}-byte ones")
    buf = _upload(torch, _buf(data), codec.device)
    dbase = None
    if _ELEM[kind].based:
        dbase = _upload(torch, _host_base(np.empty(info.n_elems, dtype=dt), base), codec.device)
    out, status = codec._elem_decompress(kind, buf, getattr(torch, np.dtype(_INT_VIEW[info.elem_bytes]).name), 0,
                                         dbase)
    _raise_first_failed(status, f"{label} frame block")
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
