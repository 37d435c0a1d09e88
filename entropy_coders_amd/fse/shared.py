"""Shared-table coding: one caller's table on the device and many small
messages coded against it (fsehip.h section 2c, fse_capi_shared.cpp)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .._lib import STATUS, FseError, NormHistogram, check, load
from ._helpers import _buf, _lay_out_streams, _p, _ptr
from .host import histogram_new, normalize

__all__ = ["SharedTable", "norm_histogram_try_from"]


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

        self.lib = load()
        self.device = torch.device(device or "cuda")
        self.table_log = int(nh.log2)
        d_nh = torch.from_numpy(np.frombuffer(bytes(nh), dtype=np.uint8).copy()).to(self.device)
        self.image = torch.zeros(int(self.lib.fsehip_shared_table_bytes()), dtype=torch.uint8, device=self.device)
        st = torch.zeros(1, dtype=torch.int32, device=self.device)
        check(self.lib.fsehip_shared_table_build(_ptr(d_nh), _ptr(self.image), _ptr(st), self._stream()),
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

        n, dev = len(bufs), self.device
        desc, d_in, d_desc, out = _lay_out_streams(torch, bufs, caps, dev)
        lens = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        return desc, d_in, d_desc, out, lens, status

    def compress(self, buffers, nstates: int = 2, out_caps=None, raw: bool = False):
        """`fsehip_compress_shared`: per message (payload bytes, payload bits)
        or the name of its status.  out_caps[i] bytes per output region
        (default `fsehip_shared_out_bytes`).  raw=True: (statuses, lengths,
        payload bits, out bytes as numpy, descriptors) for bounds checks."""
        import torch

        bufs = [_buf(x) for x in buffers]
        n = len(bufs)
        caps = ([int(self.lib.fsehip_shared_out_bytes(len(b), self.table_log)) for b in bufs]
                if out_caps is None else list(out_caps))
        desc, d_src, d_desc, out, comp_len, status = self._upload(bufs, caps)
        bits = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        check(self.lib.fsehip_compress_shared(nstates, _ptr(self.image), _ptr(d_src), _ptr(d_desc), n, _ptr(out),
                                              _ptr(comp_len), _ptr(bits), _ptr(status), self._stream()),
              "fsehip_compress_shared")
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
        check(self.lib.fsehip_decompress_shared(nstates, _ptr(self.image), _ptr(d_in), _ptr(d_desc), n, _ptr(out),
                                                _ptr(d_raw), _ptr(out_len), _ptr(status), self._stream()),
              "fsehip_decompress_shared")
        torch.cuda.synchronize(self.device)
        ho, ol, st = out.cpu().numpy(), out_len.cpu().numpy()[:n], status.cpu().numpy()[:n]
        if raw:
            return st, ol, ho, [(d.src_off, d.out_off, d.src_len, d.out_cap) for d in desc[:n]]
        return [ho[desc[i].out_off: desc[i].out_off + int(ol[i])].tobytes() if st[i] == 0 else
                STATUS.get(int(st[i]), str(int(st[i]))) for i in range(n)]
