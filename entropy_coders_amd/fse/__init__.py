"""Python mirror of the reference crate's API for this path (tests, bench).

Reference-shaped calls (host bytes in, bytes out; lib.rs:146-248,
histogram.rs:18-66) and a batched device codec over torch tensors.  All
compute goes through libfsehip.so on the GPU.  One module per section of
include/fsehip.h and per fse_capi_*.cpp; each holds its
concern's part of BlockCodec as a plain base class, whose own bases are the
concerns it calls through `self`, and the concern's host-bytes functions.
"""
from . import bits, check, core, elem, estimate, frame, host, pack, shared
from .bits import *  # noqa: F401,F403
from .check import *  # noqa: F401,F403
from .elem import *  # noqa: F401,F403
from .estimate import *  # noqa: F401,F403
from .frame import *  # noqa: F401,F403
from .host import *  # noqa: F401,F403
from .pack import *  # noqa: F401,F403
from .shared import *  # noqa: F401,F403


class BlockCodec(pack._PackCodec, check._CheckCodec, estimate._EstimateCodec, frame._FrameCodec, elem._ElemCodec,
                 core._CodecCore):
    """Batched device codec: 64 KiB blocks (configurable) over torch tensors.

    compress(src) -> CompressedBlocks (slots, lengths, sidecar, status), all
    resident on the device; decompress(cb) -> uint8 tensor.  Work is queued
    on torch's current stream.
    """


__all__ = ["BlockCodec", *host.__all__, *bits.__all__, *frame.__all__, *elem.__all__, *check.__all__,
           *estimate.__all__, *pack.__all__, *shared.__all__]
