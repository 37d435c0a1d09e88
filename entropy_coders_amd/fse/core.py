"""The batched device codec's core: parameters, stream, workspace and rank
counters, block compress and decompress, sidecar, decode tables (fsehip.h
section 2a, fse_capi.cpp).  The base every concern's class builds on."""
from __future__ import annotations

import ctypes as C

from .._lib import FrameParams, Params, check, load

__all__ = []  # BlockCodec, which the package composes, is the public name


class _CodecCore:
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

    def _frame_params(self, chunk_blocks: int = 0) -> FrameParams:
        return FrameParams(self.block_size, self.table_log, self.ckpt_interval, self.max_table_log, self.nstates,
                           chunk_blocks)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _device_index(self) -> int:
        return self.device.index if self.device.index is not None else self.torch.cuda.current_device()

    def release_workspace(self) -> None:
        """`fsehip_release_workspace` for this codec's device and torch's
        current stream: frees the decode workspace (decode tables, and the
        deferred-symbol states: 2 bytes per output byte of the last
        sidecar-less batch) after the queued work."""
        check(self.lib.fsehip_release_workspace(self._device_index(), self._stream()), "fsehip_release_workspace")

    def rank_fallbacks(self, reset: bool = False) -> dict:
        """`fsehip_rank_fallbacks` on this codec's device: tables whose atomic
        ranks failed their self-check and were rebuilt with peer-mask ranks
        (batch encoder, decode-table builds, building-block table calls)."""
        out = (C.c_uint32 * 3)()
        check(self.lib.fsehip_rank_fallbacks(self._device_index(), C.byref(out), 1 if reset else 0),
              "fsehip_rank_fallbacks")
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

    def block_bytes(self, cb: dict, b: int) -> bytes:
        """Compressed bytes of block b (host copy) -- for parity checks."""
        ln = int(cb["comp_len"][b].item())
        s = b * self.slot_bytes
        return cb["out"][s: s + ln].cpu().numpy().tobytes()
