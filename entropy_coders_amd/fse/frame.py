"""The frame: one self-describing buffer for any input (RAW / RLE fallback
per block), this library's own container (fsehip.h section 2b,
fse_capi_frame.cpp), and its host-bytes convenience functions."""
from __future__ import annotations

import ctypes as C

from .._lib import FrameInfo, FrameRange, check, load
from ._helpers import _back_to_back, _buf, _head, _p, _ptr, _raise_first_failed, _upload
from .core import _CodecCore

__all__ = ["frame_compress", "frame_decompress", "frame_decompress_range"]


class _FrameCodec(_CodecCore):
    def frame_bound(self, n: int) -> int:
        """`fsehip_frame_bound`: a capacity no frame of n bytes exceeds."""
        return int(self.lib.fsehip_frame_bound(n, self.block_size))

    def compress_frame_into(self, src, frame, frame_len, result, chunk_blocks: int = 0) -> None:
        """`fsehip_frame_compress`, no synchronisation: `frame` a uint8 device
        tensor of >= frame_bound(src.numel()) bytes (any alignment),
        `frame_len` one int64, `result` two int32 (frame status, blocks not
        stored as FSE)."""
        p = self._frame_params(chunk_blocks)
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
        a = _head(frame, 32)
        info = FrameInfo()
        check(load().fsehip_frame_read_header(_p(a), len(a), C.byref(info)), "fsehip_frame_read_header")
        return info

    def decompress_frame_into(self, frame, info: FrameInfo, out, block_status, result, chunk_blocks: int = 0) -> None:
        """`fsehip_frame_decompress`, no synchronisation: `out` >= info.n_total
        bytes (16-byte aligned), `block_status` info.n_blocks int32 or None,
        `result` two int32 (frame status, failed blocks)."""
        check(self.lib.fsehip_frame_decompress(
            C.byref(info), chunk_blocks, C.c_void_p(frame.data_ptr()), frame.numel(), C.c_void_p(out.data_ptr()),
            out.numel(), _ptr(block_status), C.c_void_p(result.data_ptr()), self._stream()), "fsehip_frame_decompress")

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
            C.c_void_p(out.data_ptr()), out.numel(), _ptr(range_status), C.c_void_p(result.data_ptr()),
            self._stream()), "fsehip_frame_decompress_ranges")

    def decompress_frame_ranges(self, frame, ranges, chunk_blocks: int = 0):
        """Decode the raw byte ranges [(src_off, len), ...] of a frame (a uint8
        device tensor) without decoding the rest.  The ranges are packed back
        to back into one uint8 tensor; returns (list of views of it, one per
        range, and the int32 range statuses).  Raises FseError for a
        frame-level error (BAD_FRAME)."""
        t = self.torch
        info = self.frame_info(frame)
        packed, at = _back_to_back(ranges)
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


def frame_compress(data, block_size: int = 65536, table_log: int = 0, ckpt_interval: int = 128, nstates: int = 2,
                   device=None) -> bytes:
    """Compress any host buffer (bytes, numpy; empty included) into one frame
    (fsehip.h section 2b) on the GPU; copies through torch."""
    import torch

    codec = _FrameCodec(block_size, table_log, ckpt_interval, device, nstates)
    return codec.compress_frame(_upload(torch, _buf(data), codec.device)).cpu().numpy().tobytes()


def frame_decompress(data, device=None) -> bytes:
    """Decode a frame held in host memory; raises FseError on a frame-level
    error (BAD_FRAME) or with the first failed block's status."""
    import torch

    codec = _FrameCodec(device=device)
    codec.frame_info(_buf(data))  # not a frame: BAD_FRAME before any device work
    out, status = codec.decompress_frame(_upload(torch, _buf(data), codec.device))
    _raise_first_failed(status, "frame block")
    return out.cpu().numpy().tobytes()


def frame_decompress_range(data, offset: int, length: int, device=None) -> bytes:
    """Raw bytes [offset, offset + length) of a frame held in host memory;
    raises FseError as BlockCodec.decompress_frame_range.  The whole frame is
    uploaded: sending only the header, the directory and the records the
    range needs is out of scope here."""
    import torch

    codec = _FrameCodec(device=device)
    codec.frame_info(_buf(data))  # not a frame: BAD_FRAME before any device work
    frame = _upload(torch, _buf(data), codec.device)
    return codec.decompress_frame_range(frame, offset, length).cpu().numpy().tobytes()
