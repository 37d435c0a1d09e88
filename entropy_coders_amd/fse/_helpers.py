"""Small private helpers every module of the package shares: host buffers
and their pointers, the head bytes of a container, a tensor's pointer, the
upload and the checks of the host-bytes convenience functions."""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from .._lib import FseError, StreamDesc

__all__ = []  # nothing here is public

# the integer view a host array of each item size travels as
_INT_VIEW = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}

_tls = threading.local()


def _buf(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _out(cap: int) -> np.ndarray:
    """A per-thread output buffer of >= cap bytes, reused across calls (the
    calls return copies): allocating a fresh 16 MiB array per call costs
    more than a small decode."""
    b = getattr(_tls, "out", None)
    if b is None or len(b) < cap:
        b = np.empty(max(cap, 1), dtype=np.uint8)
        _tls.out = b
    return b


def take(buf, lo: int, hi: int) -> bytes:
    """buf[lo:hi] of bytes, a numpy array or a tensor as host bytes."""
    if hasattr(buf, "data_ptr"):  # a torch tensor
        return buf[lo:hi].cpu().numpy().tobytes()
    return bytes(memoryview(buf)[lo:hi])


def _head(buf, n: int) -> np.ndarray:
    """The first n bytes of a container (as `take`) as the uint8 array a read-header call takes."""
    return np.frombuffer(take(buf, 0, n), dtype=np.uint8)


def _ptr(x):
    """The device pointer of a tensor, or None (a null pointer) for None."""
    return C.c_void_p(x.data_ptr()) if x is not None else None


def _back_to_back(ranges) -> tuple:
    """(offset, count) pairs as (offset, count, destination) triples packed back to back, and their total count."""
    packed, at = [], 0
    for s, n in ranges:
        packed.append((s, n, at))
        at += n
    return packed, at


def _pack_prefix(versioned: bool) -> str:
    """The C names' prefix of the pack frame's calls or of the versioned pack's."""
    return "fsehip_vpack_" if versioned else "fsehip_pack_"


def _upload(torch, a: np.ndarray, device):
    """A copy of a host array on the device."""
    return torch.from_numpy(a.copy()).to(device)


def _lay_out_streams(torch, bufs, caps, dev) -> tuple:
    """Inputs back to back at 16-byte aligned offsets, output regions of caps[i] bytes 64 bytes apart and filled
    with 0xA5: (descriptors, and on the device the inputs, the descriptors and the output regions)."""
    desc = (StreamDesc * max(len(bufs), 1))()
    so = oo = 0
    for i, b in enumerate(bufs):
        desc[i] = StreamDesc(so, oo, len(b), caps[i])
        so += (len(b) + 15) // 16 * 16
        oo += (caps[i] + 15) // 16 * 16 + 64
    host = np.zeros(max(so, 16), dtype=np.uint8)
    for i, b in enumerate(bufs):
        host[desc[i].src_off: desc[i].src_off + len(b)] = b
    return (desc, torch.from_numpy(host).to(dev), _upload(torch, np.frombuffer(bytes(desc), dtype=np.uint8), dev),
            torch.full((max(oo, 16),), 0xA5, dtype=torch.uint8, device=dev))


def _raise_first_failed(status, what: str) -> None:
    """FseError with the status of the first failed entry of a device status tensor, named `what` N."""
    st = status.cpu().numpy()
    if st.any():
        b = int(np.flatnonzero(st)[0])
        raise FseError(int(st[b]), f"{what} {b}")
