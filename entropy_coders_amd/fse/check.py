"""The check record and sealed buffers: a CRC-32 (zlib's) per check block
of the content, in a record of its own in front of an unchanged container
(fsehip.h section 2f, fse_capi_check.cpp), and their host-bytes
convenience functions."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .._lib import SEALED_KINDS, CheckInfo, FseError, check, load
from ._helpers import _INT_VIEW, _back_to_back, _buf, _head, _p, _raise_first_failed, _upload
from .elem import _ELEM, _host_base
from .estimate import _EstimateCodec, estimate_choose

__all__ = ["sealed_compress", "sealed_decompress", "crc32", "crc32_combine", "CheckInfo"]


class _CheckCodec(_EstimateCodec):
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
        a = _head(record, 32)
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
        info = _CheckCodec.check_info(buf)
        a = _head(buf, 32 + 4 * info.n_cb + 48)
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
        packed, at = _back_to_back(ranges)
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

    codec = _CheckCodec(block_size, table_log, ckpt_interval, device, nstates)
    if kind == "frame":
        a = _buf(data) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    else:
        a = np.ascontiguousarray(data) if isinstance(data, np.ndarray) or kind != "auto" else _buf(data)
        if a.dtype.itemsize not in _INT_VIEW:
            raise ValueError(f"item size {a.dtype.itemsize}: 1, 2, 4 or 8 bytes")
        if kind == "diff" or (kind == "auto" and base is not None):
            base = _upload(torch, _host_base(a, base), codec.device)
        a = a.reshape(-1).view(_INT_VIEW[a.dtype.itemsize])
    src = _upload(torch, a, codec.device)
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

    codec = _CheckCodec(device=device)
    info, kind, off = codec.sealed_info(_buf(blob))  # not a sealed buffer: BAD_FRAME before any device work
    buf = _upload(torch, _buf(blob), codec.device)
    dt = None if dtype is None else np.dtype(dtype)
    dbase = None
    if kind == "diff":
        if base is None:
            raise ValueError("a sealed diff buffer needs base=")
        b = np.ascontiguousarray(base).reshape(-1)
        if b.dtype.itemsize not in _INT_VIEW:
            raise ValueError(f"item size {b.dtype.itemsize}: 1, 2, 4 or 8 bytes")
        dbase = _upload(torch, b.view(_INT_VIEW[b.dtype.itemsize]), codec.device)
    out, status, check_status, result = codec.decompress_sealed(buf, None, with_result=True, base=dbase)
    if dt is not None and dt.itemsize != out.element_size():
        raise ValueError(f"dtype {dt} has {dt.itemsize}-byte items, the sealed buffer holds {out.element_size()}-byte ones")
    _raise_first_failed(status, f"sealed {kind} block")
    _raise_first_failed(check_status, f"sealed {kind} check block")
    check(int(result.cpu().numpy()[0]), f"sealed {kind} content")
    host = out.cpu().numpy()
    if kind == "frame" and dt is None:
        return host.tobytes()
    return host.view(dt) if dt is not None else host
