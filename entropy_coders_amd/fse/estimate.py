"""The size estimate (fsehip.h sections 2g and 2i, fse_capi_estimate.cpp):
the length each container would have, from the block histograms of its
image and the encoder's own normalisation, and the automatic choice among
compress_frame / compress_planes / compress_delta and, for a caller who
passes the tensor's base, compress_diff.  Kinds are "frame", "planes",
"delta" (or 0, 1, 2) and, with base=, "diff" (or 4)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .._lib import EST_NONE, KIND_DIFF, KIND_PACK, KIND_SEALED, KIND_SPACK, KIND_VPACK, KINDS, FseError, check, load
from ._helpers import _INT_VIEW, _buf, _head, _p, _upload
from .elem import _ELEM, _ElemCodec, _elem_decompress, _host_base
from .frame import _FrameCodec, frame_decompress

__all__ = ["auto_compress", "auto_decompress", "container_kind", "estimate_choose", "log2q8"]

# fsehip_estimate_base's five entries by FSEHIP_KIND_*: entry 3 (sealed) is no choice of container
_BASE_KINDS = KINDS + (None, "diff")
# fsehip_container_kind's names past KINDS
_CONTAINER_KINDS = {KIND_SEALED: "sealed", KIND_DIFF: "diff", KIND_PACK: "pack", KIND_VPACK: "vpack",
                    KIND_SPACK: "spack"}


class _EstimateCodec(_FrameCodec, _ElemCodec):
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
    elif isinstance(est, dict):
        est = [est.get(name, EST_NONE) for name in KINDS]
    based = len(est) == 5
    arr = (C.c_uint64 * (5 if based else 3))(*[int(v) for v in est])
    k = (load().fsehip_estimate_choose_base if based else load().fsehip_estimate_choose)(C.byref(arr))
    if k < 0:
        raise ValueError("no estimate to choose from")
    return (_BASE_KINDS if based else KINDS)[k]


def container_kind(buf) -> str:
    """`fsehip_container_kind`: "frame", "planes", "delta", "sealed", "diff", "pack", "vpack" or "spack" from
    the magic of a container given as bytes, a numpy array or a tensor (its
    first 4 bytes come to the host); raises FseError (BAD_FRAME) for anything
    else."""
    a = _head(buf, 4)
    k = load().fsehip_container_kind(_p(a), len(a))
    if k < 0:
        raise FseError(k, "fsehip_container_kind")
    return _CONTAINER_KINDS.get(k) or KINDS[k]


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
    codec = _EstimateCodec(block_size, table_log, ckpt_interval, device, nstates)
    src = _upload(torch, a.reshape(-1).view(_INT_VIEW[a.dtype.itemsize]), codec.device)
    dbase = None if base is None else _upload(torch, _host_base(a, base), codec.device)
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
