"""Packs, all three flavours (fsehip.h sections 2j, 2k and 2l;
fse_capi_pack.cpp, fse_capi_spack.cpp).  The pack frame: many tensors in one
container, one transform launch over all of them each way around one frame
call.  A member is coded as "planes" or "delta" (both at 1-, 2-, 4- and
8-byte elements); dtypes and shapes stay with the caller.

With bases= the same calls write and read the versioned pack: a member with
a base may be coded as "diff", its zigzag difference against the base
tensor.  THE CONTAINER DOES NOT IDENTIFY ITS BASES.  The sealed pack is
further down."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .._lib import (KIND_DIFF, KIND_VPACK, MCHECK_BASES, FrameInfo, FseError, McheckInfo, PackInfo, PackMember, check,
                    load)
from ._helpers import _INT_VIEW, _buf, _p, _pack_prefix, _ptr, _raise_first_failed, _upload, take
from .core import _CodecCore

__all__ = ["pack_compress", "pack_decompress", "pack_info", "PackHead",
           "pack_sealed_compress", "pack_sealed_decompress", "pack_sealed_info", "McheckInfo", "MCHECK_BASES"]


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


class _PackCodec(_CodecCore):
    _PACK_KINDS = {"planes": 1, "delta": 2}
    _VPACK_KINDS = {"planes": 1, "delta": 2, "diff": KIND_DIFF}

    def _pack_fn(self, name: str, versioned: bool):
        return getattr(self.lib, _pack_prefix(versioned) + name)

    def _pack_call(self, name: str, barr, at: int, *args) -> None:
        """fsehip_pack_<name>(*args); with `barr`, a versioned pack's array of
        base pointers, fsehip_vpack_<name> with it as argument `at`."""
        versioned = barr is not None
        if versioned:
            args = args[:at] + (barr,) + args[at:]
        check(self._pack_fn(name, versioned)(*args), _pack_prefix(versioned) + name)

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

    def _pack_list(self, tensors, kinds, bases) -> tuple:
        """(members, n, versioned, base pointers or None) of a list of tensors: pack_bases, pack_members."""
        n, versioned, barr = len(tensors), bases is not None, None
        if versioned:
            kinds, barr = self.pack_bases(tensors, bases, kinds)
        return self.pack_members(tensors, kinds, versioned), n, versioned, barr

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
        members, n, versioned, barr = self._pack_list(tensors, kinds, bases)
        image = t.empty(int(self._pack_fn("image_bytes", versioned)(members, n)), dtype=t.uint8, device=self.device)
        scratch = self._pack_transform_scratch(members, n, versioned)
        self._pack_call("split", barr, 2, members, n, C.c_void_p(image.data_ptr()), C.c_void_p(scratch.data_ptr()),
                        scratch.numel(), self._stream())
        return image

    def pack_merge(self, image, outs, kinds=None, bases=None):
        """The members of a pack image into the tensors `outs` (their sizes
        and dtypes say the list): fsehip_pack_merge; with `bases` the
        versioned pack's, fsehip_vpack_merge (an out may be its base itself)."""
        members, n, versioned, barr = self._pack_list(outs, kinds, bases)
        scratch = self._pack_transform_scratch(members, n, versioned)
        self._pack_call("merge", barr, 2, members, n, C.c_void_p(image.data_ptr()), C.c_void_p(scratch.data_ptr()),
                        scratch.numel(), self._stream())
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
        self._pack_call("compress", bases, 3, C.byref(p), members, n, C.c_void_p(scratch.data_ptr()), scratch.numel(),
                        C.c_void_p(out.data_ptr()), out.numel(), C.c_void_p(out_len.data_ptr()),
                        C.c_void_p(result.data_ptr()), self._stream())

    def _pack_compress(self, sealed: bool, tensors, kinds, bases, chunk_blocks: int, check_bases: bool = True):
        """compress_pack or, `sealed`, compress_pack_sealed."""
        t = self.torch
        members, n, versioned, barr = self._pack_list(tensors, kinds, bases)
        if sealed:
            bound = self.pack_sealed_bound(members, n, versioned)
            need = self.pack_sealed_scratch_bytes(members, n, versioned)
        else:
            bound, need = self.pack_bound(members, n, versioned), self.pack_scratch_bytes(members, n, versioned)
        if not bound or not need:
            raise FseError(-14, "fsehip_spack_bound" if sealed else "fsehip_pack_bound")
        scratch = t.empty(need, dtype=t.uint8, device=self.device)
        out = t.empty(bound, dtype=t.uint8, device=self.device)
        out_len = t.zeros(1, dtype=t.int64, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        if sealed:
            self.compress_pack_sealed_into(members, n, scratch, out, out_len, result, chunk_blocks, barr, check_bases)
        else:
            self.compress_pack_into(members, n, scratch, out, out_len, result, chunk_blocks, barr)
        return out[: int(out_len.item())]

    def compress_pack(self, tensors, kinds=None, chunk_blocks: int = 0, bases=None):
        """Compress a list of contiguous device tensors into one pack frame: a
        uint8 device tensor of its exact length.  `kinds`: None (all
        "planes"), one name or one per tensor.  With `bases` (one entry per
        tensor: None, or a contiguous device tensor of the same element size
        and count) the output is a versioned pack, and the kinds default to
        "diff" where a base is given and "planes" where not.  One
        synchronisation, to read the length."""
        return self._pack_compress(False, tensors, kinds, bases, chunk_blocks)

    @staticmethod
    def pack_info(buf):
        """The head of a pack frame or a versioned pack given as bytes, a
        numpy array or a tensor (its 32 + 16 n + 32 head bytes come to the
        host): a PackHead with `info` (PackInfo), `members` (the PackMember
        array, pointers null), `inner` (the frame's FrameInfo), the lists
        `kinds`, `elem_bytes` and `n_elems`, and `container`, "pack" or
        "vpack"; raises FseError (BAD_FRAME) otherwise."""
        lib = load()
        info, inner = PackInfo(), FrameInfo()
        a = np.frombuffer(take(buf, 0, 32), dtype=np.uint8)
        versioned = lib.fsehip_container_kind(_p(a), len(a)) == KIND_VPACK
        prefix = _pack_prefix(versioned)
        check(getattr(lib, prefix + "read_header")(_p(a), len(a), C.byref(info)), prefix + "read_header")
        n = info.n_members
        a = np.frombuffer(take(buf, 0, 32 + 16 * n + 32), dtype=np.uint8)
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

    def _pack_decode_call(self, buf, head, indices, selected: bool, outs, scratch, status, result, chunk_blocks,
                          bases) -> None:
        """The decompress call for all members (`status` per block) or,
        `selected`, the decompress_members call for `indices` (per index)."""
        outs = self._pack_outs(head, indices, [o.dtype for o in outs], outs)
        members = self._pack_point(head, indices, outs)
        sel = ((C.c_uint32 * max(len(indices), 1))(*indices), len(indices)) if selected else ()
        barr = self._pack_decode_bases(head, indices, bases) if head.container == "vpack" else None
        self._pack_call("decompress_members" if selected else "decompress", barr, 2, C.byref(head.info), members,
                        C.byref(head.inner), chunk_blocks, C.c_void_p(buf.data_ptr()), buf.numel(), *sel,
                        C.c_void_p(scratch.data_ptr()), scratch.numel(), _ptr(status), C.c_void_p(result.data_ptr()),
                        self._stream())

    def decompress_pack_into(self, buf, head, outs, scratch, block_status, result, chunk_blocks: int = 0,
                             bases=None) -> None:
        """fsehip_pack_decompress, no synchronisation: `head` from pack_info,
        `outs` one contiguous tensor per member (element size and count the
        table's), `scratch` >= pack_scratch_bytes (16-byte aligned),
        `block_status` head.inner.n_blocks int32 or None, `result` two int32.
        A versioned pack (fsehip_vpack_decompress; its scratch is
        pack_scratch_bytes(..., versioned=True)) takes `bases`, one entry per
        member or a dict by index; an out may be its base itself."""
        self._pack_decode_call(buf, head, list(range(head.info.n_members)), False, outs, scratch, block_status, result,
                               chunk_blocks, bases)

    def decompress_pack_members_into(self, buf, head, indices, outs, scratch, member_status, result,
                                     chunk_blocks: int = 0, bases=None) -> None:
        """fsehip_pack_decompress_members, no synchronisation: `outs` one
        tensor per index, `scratch` >= pack_members_scratch_bytes,
        `member_status` len(indices) int32 or None, `result` two int32.  A
        versioned pack (fsehip_vpack_decompress_members) takes `bases`, a list
        with one entry per index or a dict by member index: the selected diff
        members' are needed."""
        self._pack_decode_call(buf, head, [int(i) for i in indices], True, outs, scratch, member_status, result,
                               chunk_blocks, bases)

    @staticmethod
    def _pack_selection(head, indices) -> tuple:
        """(member indices, whether a selection): all for `indices` None, else `indices`, none twice."""
        if indices is None:
            return list(range(head.info.n_members)), False
        indices = [int(i) for i in indices]
        if len(set(indices)) != len(indices):
            raise ValueError("a member is selected twice")
        return indices, True

    def _decompress_pack(self, buf, indices, dtypes, chunk_blocks: int, bases, outs):
        """decompress_pack (`indices` None) or decompress_pack_members."""
        t = self.torch
        head = self.pack_info(buf)
        indices, selected = self._pack_selection(head, indices)
        n, versioned = head.info.n_members, head.container == "vpack"
        if versioned and not selected:
            self._pack_decode_bases(head, indices, bases)  # the argument errors, ahead of any allocation
        outs = self._pack_outs(head, indices, dtypes, outs)
        if selected:
            if versioned:
                self._pack_decode_bases(head, indices, bases)
            need = max(self.pack_members_scratch_bytes(head.members, n, indices, versioned), 16)
        else:
            need = self.pack_scratch_bytes(head.members, n, versioned)
        scratch = t.empty(need, dtype=t.uint8, device=self.device)
        status = t.zeros(len(indices) if selected else head.inner.n_blocks, dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        self._pack_decode_call(buf, head, indices, selected, outs, scratch, status, result, chunk_blocks, bases)
        check(int(result[0].item()), "pack frame")
        return outs, status

    def decompress_pack(self, buf, dtypes, chunk_blocks: int = 0, bases=None, outs=None):
        """Decode a pack frame or a versioned pack (a uint8 device tensor)
        into one 1-D tensor per member; `dtypes` is one dtype or one per
        member, each of the member's element size (ValueError otherwise).
        A versioned pack with diff members needs `bases` (one entry per
        member, None where there is none; ValueError without).  `outs`: the
        destinations, fresh tensors by default; outs=bases, or the same
        tensors in both, decodes in place.  Returns (tensors, block_status);
        raises FseError for a frame-level error (BAD_FRAME)."""
        return self._decompress_pack(buf, None, dtypes, chunk_blocks, bases, outs)

    def decompress_pack_members(self, buf, indices, dtypes, chunk_blocks: int = 0, bases=None, outs=None):
        """Decode only the members `indices` of a pack frame or a versioned
        pack (only the blocks they cover are decoded).  `bases`: a list with
        one entry per index or a dict by member index, covering the selected
        diff members of a versioned pack; `outs`: the destinations, fresh
        tensors by default.  Returns (tensors, member_status); raises FseError
        for a frame-level error."""
        return self._decompress_pack(buf, indices, dtypes, chunk_blocks, bases, outs)

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
        members, n, versioned, barr = self._pack_list(tensors, kinds, bases)
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
        return self._pack_compress(True, tensors, kinds, bases, chunk_blocks, check_bases)

    @staticmethod
    def pack_sealed_info(buf):
        """The head of a sealed pack given as bytes, a numpy array or a tensor:
        (record, head) with `record` the McheckInfo of the member check record
        (`record.flags & 1`: base CRCs recorded) and `head` the PackHead of the
        pack behind it, which starts at byte 32 + 8 n; raises FseError
        (BAD_FRAME) otherwise."""
        lib = load()
        a = np.frombuffer(take(buf, 0, 32), dtype=np.uint8)
        rec = McheckInfo()
        check(lib.fsehip_mcheck_read_header(_p(a), len(a), C.byref(rec)), "fsehip_mcheck_read_header")
        off = 32 + 8 * rec.n_members
        a = np.frombuffer(take(buf, 0, off + 32), dtype=np.uint8)
        versioned, inner_off = C.c_uint32(0), C.c_uint64(0)
        check(lib.fsehip_spack_read_header(_p(a), len(a), C.byref(rec), C.byref(versioned), C.byref(inner_off)),
              "fsehip_spack_read_header")
        head = _PackCodec.pack_info(np.frombuffer(take(buf, off, off + 32 + 16 * rec.n_members + 32), dtype=np.uint8))
        if (head.container == "vpack") != bool(versioned.value):
            raise FseError(-19, "sealed pack")
        return rec, head

    def _pack_sealed_call(self, buf, rec, head, indices, selected, outs, scratch, status, result, member_check,
                          base_check, check_result, chunk_blocks, bases) -> None:
        versioned = head.container == "vpack"
        outs = self._pack_outs(head, indices, [o.dtype for o in outs], outs)
        members = self._pack_point(head, indices, outs)
        barr = self._pack_decode_bases(head, indices, bases) if versioned else None
        sel = ((C.c_uint32 * max(len(indices), 1))(*indices), len(indices)) if selected else ()
        name = "fsehip_spack_decompress_members" if selected else "fsehip_spack_decompress"
        check(getattr(self.lib, name)(
            C.byref(rec), C.byref(head.info), int(versioned), members, barr, C.byref(head.inner), chunk_blocks,
            _ptr(buf), buf.numel(), *sel, _ptr(scratch), scratch.numel(), _ptr(status), _ptr(result),
            _ptr(member_check), _ptr(base_check), _ptr(check_result), self._stream()), name)

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

    def _decompress_pack_sealed(self, buf, indices, dtypes, bases, outs, chunk_blocks: int, with_result: bool):
        """decompress_pack_sealed (`indices` None) or decompress_pack_members_sealed."""
        t = self.torch
        rec, head = self.pack_sealed_info(buf)
        indices, selected = self._pack_selection(head, indices)
        n, versioned = head.info.n_members, head.container == "vpack"
        outs = self._pack_outs(head, indices, dtypes, outs)
        if selected:
            need = max(self.pack_sealed_members_scratch_bytes(head.members, n, indices, versioned), 16)
        else:
            need = self.pack_sealed_scratch_bytes(head.members, n, versioned)
        scratch = t.empty(need, dtype=t.uint8, device=self.device)
        status = t.zeros(len(indices) if selected else head.inner.n_blocks, dtype=t.int32, device=self.device)
        result = t.zeros(2, dtype=t.int32, device=self.device)
        mcheck = t.zeros(len(indices), dtype=t.int32, device=self.device)
        bcheck = t.zeros(len(indices), dtype=t.int32, device=self.device)
        cres = t.zeros(4, dtype=t.int32, device=self.device)
        self._pack_sealed_call(buf, rec, head, indices, selected, outs, scratch, status, result, mcheck, bcheck, cres,
                               chunk_blocks, bases)
        check(int(result[0].item()), "pack frame")
        if int(cres[0].item()) == -19:
            raise FseError(-19, "member check record")
        return (outs, status, mcheck, bcheck, cres) if with_result else (outs, status, mcheck, bcheck)

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
        return self._decompress_pack_sealed(buf, None, dtypes, bases, outs, chunk_blocks, with_result)

    def decompress_pack_members_sealed(self, buf, indices, dtypes, bases=None, outs=None, chunk_blocks: int = 0,
                                       with_result: bool = False):
        """Decode only the members `indices` of a sealed pack, as
        decompress_pack_members; whole members are verified, and the gate
        looks at the selected members' bases.  Returns (tensors,
        member_status, member_check, base_check), one entry per index."""
        return self._decompress_pack_sealed(buf, indices, dtypes, bases, outs, chunk_blocks, with_result)


def pack_info(buf):
    """`BlockCodec.pack_info`: the head of a pack frame (fsehip.h section 2j)."""
    return _PackCodec.pack_info(buf)


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
        tensors.append(_upload(torch, a.reshape(-1).view(_INT_VIEW[a.dtype.itemsize]), device))
    return tensors


def _pack_host_decode(sealed: bool, blob, head, dtypes, bases, device) -> tuple:
    """What pack_decompress and pack_sealed_decompress share: the dtype checks, the uploads and the decode.
    Returns (numpy dtypes, what the codec's decompress_pack or decompress_pack_sealed returned)."""
    import torch

    n = head.info.n_members
    dts = [np.dtype(d) for d in (dtypes if isinstance(dtypes, (list, tuple)) else [dtypes] * n)]
    if len(dts) != n:
        raise ValueError(f"{len(dts)} dtypes for {n} members")
    for m, dt in enumerate(dts):
        if dt.itemsize != head.elem_bytes[m]:
            raise ValueError(f"dtype {dt} has {dt.itemsize}-byte items, member {m} holds {head.elem_bytes[m]}-byte ones")
    codec = _PackCodec(device=device)
    buf = _upload(torch, _buf(blob), codec.device)
    bases = None if bases is None else _pack_host_tensors(bases, "base", codec.device, optional=True)
    decode = codec.decompress_pack_sealed if sealed else codec.decompress_pack
    return dts, decode(buf, [getattr(torch, np.dtype(_INT_VIEW[w]).name) for w in head.elem_bytes], bases=bases)


def pack_compress(arrays, kinds=None, block_size: int = 65536, table_log: int = 0, ckpt_interval: int = 128,
                  nstates: int = 2, device=None, bases=None) -> bytes:
    """Compress a list of numpy arrays of item size 1, 2, 4 or 8 into one pack
    frame on the GPU; copies through torch.  `kinds`: None (all "planes"), one
    name or one per array.  With `bases` (one entry per array: None or an
    array of the same item size and count) the output is a versioned pack, as
    BlockCodec.compress_pack.  The element widths are stored, dtypes and
    shapes are not."""
    codec = _PackCodec(block_size, table_log, ckpt_interval, device, nstates)
    tensors = _pack_host_tensors(arrays, "member", codec.device)
    bases = None if bases is None else _pack_host_tensors(bases, "base", codec.device, optional=True)
    return codec.compress_pack(tensors, kinds, bases=bases).cpu().numpy().tobytes()


def pack_decompress(blob, dtypes, device=None, bases=None) -> list:
    """Decode a pack frame or a versioned pack held in host memory into one
    1-D numpy array per member; `dtypes` is one dtype or one per member (each
    of the member's item size); `bases`: one entry per member, None or the
    array a diff member was coded against; raises FseError on a frame-level
    error or with the first failed block's status."""
    head = _PackCodec.pack_info(_buf(blob))  # not a pack: BAD_FRAME before any device work
    dts, (outs, status) = _pack_host_decode(False, blob, head, dtypes, bases, device)
    _raise_first_failed(status, "pack frame block")
    return [o.cpu().numpy().view(dt) for o, dt in zip(outs, dts)]


def pack_sealed_info(buf):
    """`BlockCodec.pack_sealed_info`: the record and the head of a sealed pack (fsehip.h section 2l)."""
    return _PackCodec.pack_sealed_info(buf)


def pack_sealed_compress(arrays, kinds=None, bases=None, check_bases: bool = True, block_size: int = 65536,
                         table_log: int = 0, ckpt_interval: int = 128, nstates: int = 2, device=None) -> bytes:
    """pack_compress with the member check record in front (a sealed pack,
    fsehip.h section 2l); with `bases` and `check_bases` the record holds the
    diff members' base CRCs as well."""
    codec = _PackCodec(block_size, table_log, ckpt_interval, device, nstates)
    tensors = _pack_host_tensors(arrays, "member", codec.device)
    bases = None if bases is None else _pack_host_tensors(bases, "base", codec.device, optional=True)
    return codec.compress_pack_sealed(tensors, kinds, bases=bases, check_bases=check_bases).cpu().numpy().tobytes()


def pack_sealed_decompress(blob, dtypes, bases=None, device=None) -> list:
    """Decode a sealed pack held in host memory as pack_decompress does a
    pack, and verify it: raises FseError("CHECKSUM") naming the members whose
    base does not match the record (nothing was decoded then) or, failing
    that, the members whose content does not; BAD_FRAME for a damaged head;
    the first failed block's status otherwise."""
    rec, head = _PackCodec.pack_sealed_info(_buf(blob))  # not a sealed pack: BAD_FRAME before any device work
    dts, (outs, status, mcheck, bcheck) = _pack_host_decode(True, blob, head, dtypes, bases, device)
    bad_base = np.flatnonzero(bcheck.cpu().numpy())
    if bad_base.size:
        raise FseError(-21, f"sealed pack: base of member(s) {bad_base.tolist()} differs from the recorded base; "
                            "nothing was decoded")
    _raise_first_failed(status, "pack frame block")
    bad = np.flatnonzero(mcheck.cpu().numpy())
    if bad.size:
        raise FseError(-21, f"sealed pack: content of member(s) {bad.tolist()}")
    return [o.cpu().numpy().view(dt) for o, dt in zip(outs, dts)]
