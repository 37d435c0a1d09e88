"""Stream order of the device entry points: every fsehip_* call is
"asynchronous on a HIP stream" (include/fsehip.h), and BlockCodec queues on
torch's current stream.  Each case here runs "behind a gate": on a fresh
non-blocking side stream S a bounded delay is enqueued, then the copies that
put the real inputs over benign poison (zeros for what a decoder reads, a
constant byte for what an encoder reads, 0xA5 / -99 and guard bands for
outputs), then a whole chain of library calls with no host synchronisation
in between.  The host then asserts that the gate has not passed yet: every
call returned while its inputs did not exist.  A launch on any other stream
runs during the gate on the poison and leaves wrong bytes or a status; a
host read of device data sees the poison; a host wait for the stream fails
the assert.  Expected results come from the CPU oracle, tests/frame_ref.py or
the raw input, never from the library.

The gate is torch.cuda._sleep, timed with events by the `warm` fixture, which
also runs every chain once ungated on S (results checked): that grows the
per-(device, stream) workspaces, so no growth synchronisation falls into a
gated pass, and gives the host enqueue time of each chain.  The gate is 20x
the longest enqueue time, at least GATE_FLOOR_MS, at most 1 s.  Right before a
gated pass the chain runs once on the poison alone, so that the workspace
holds what the poison gives (failure statuses) and not the warm-up pass's
right answers: a launch on another stream that reads the scratch then shows.

Measured on an MI355X: the chains enqueue in 0.02 to 0.65 ms, so the gate is
the 50 ms floor, and the file runs in under 4 s.
"""
import ctypes as C
import time

import numpy as np
import pytest

import frame_ref as R
from oracle import oracle as O
from test_gpu_bits_device import masked, model_stack, model_stream, random_widths
from test_gpu_frame_ranges import expected, single_ranges
from test_gpu_guard_bands import FILL, assert_guards, g8, g32, g64, ptr

gpu = pytest.mark.gpu

BLOCK, CKPT = 4096, 128
N_BLOCKS, TAIL = 40, 333
SRC_POISON = 7          # the constant byte an encoder's source holds before the upload
A5, F32, F64 = FILL["uint8"], FILL["int32"], FILL["int64"]
GATE_FACTOR, GATE_FLOOR_MS, GATE_CAP_MS = 20, 50.0, 1000.0
PIN_BUFS = 8            # kPinBufs (csrc/fse_workspace.h): staging buffers of the ranges call per workspace


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


# ---------------------------------------------------------------- host data
def lut_blocks(seed, block, n_blocks, tail):
    sizes = [block] * n_blocks + ([tail] if tail else [])
    return [O.generate(0, 0.155, seed, b, s) for b, s in enumerate(sizes)]


def frame_source(seed, n_blocks=N_BLOCKS, tail=TAIL):
    """LUT p = 0.155 blocks, block 1 random bytes (stored RAW), block 2 all zeros (RLE)."""
    blocks = lut_blocks(seed, BLOCK, n_blocks, tail)
    blocks[1] = np.random.default_rng(seed).integers(0, 256, BLOCK, dtype=np.uint8)
    blocks[2] = np.zeros(BLOCK, dtype=np.uint8)
    raw = np.concatenate(blocks)
    raw.setflags(write=False)
    return raw


def valid_checkpoints(n, ckpt, nstates):
    """Entries of a block's sidecar row that are defined for n raw bytes."""
    pm = n - 1 if nstates == 1 else ((n - 3) // 2 if n & 1 else n // 2 - 1)
    return pm // ckpt + 1


def host_slots(comp, slot_bytes):
    """The slot array and comp_len of blocks given as compressed bytes."""
    slots = np.zeros(len(comp) * slot_bytes, dtype=np.uint8)
    for b, c in enumerate(comp):
        slots[b * slot_bytes: b * slot_bytes + len(c)] = np.frombuffer(c, dtype=np.uint8)
    return slots, np.array([len(c) for c in comp], dtype=np.int32)


def pinned(torch, a):
    return torch.from_numpy(np.array(a)).pin_memory()


def stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


class Chain:
    """One case: host data and expected results (__init__, no GPU), device
    buffers (alloc), poison (default stream), upload and enqueue (current
    stream, no synchronisation), check (after the stream's synchronise).
    enqueue(step9) calls step9() where the host must still be ahead of the
    gate: after its last call unless the case says otherwise."""

    probe = None  # in a gated pass: whether the gate has passed (its event's query)

    def alloc(self, torch):
        raise NotImplementedError

    def poison(self):
        raise NotImplementedError

    def upload(self):
        for dst, src in self.uploads:
            dst.copy_(src, non_blocking=True)

    def enqueue(self, step9):
        raise NotImplementedError

    def check(self):
        raise NotImplementedError


# ---------------------------------------------------------------- 1. the block path
class BlockChain(Chain):
    def __init__(self, nstates, table_log, block, n_blocks, sidecar_rebuild=True):
        self.nstates, self.table_log, self.block = nstates, table_log, block
        self.rebuild = sidecar_rebuild
        blocks = lut_blocks(0x5EED0500 + block + nstates, block, n_blocks, TAIL)
        self.sizes = [len(s) for s in blocks]
        self.nb = len(blocks)
        self.raw = np.concatenate(blocks)
        self.want = [O.compress2(s, table_log or None) if nstates == 2 else O.compress(s) for s in blocks]
        self.lens = np.array([len(w[0]) for w in self.want], dtype=np.int64)
        self.offs = np.cumsum(self.lens) - self.lens
        self.packed = np.frombuffer(b"".join(w[0] for w in self.want), dtype=np.uint8)

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        self.torch = torch
        c = self.codec = BlockCodec(block_size=self.block, table_log=self.table_log, ckpt_interval=CKPT,
                                    nstates=self.nstates)
        nb, n = self.nb, len(self.raw)
        assert c.n_blocks(n) == nb
        self.src = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.uploads = [(self.src, pinned(torch, self.raw))]
        G = self.G = {}  # name -> (whole, view, fill)

        def g(name, make, count, fill):
            G[name] = make(torch, count) + (fill,)
            return G[name][1]

        self.cb = {"n_total": n, "out": g("slots", g8, nb * c.slot_bytes, A5), "comp_len": g("comp_len", g32, nb, F32),
                   "payload_bits": g("payload_bits", g32, nb, F32),
                   "sidecar": g("sidecar", g64, nb * c.side_per_block, F64), "status": g("enc status", g32, nb, F32)}
        self.len64 = torch.zeros(nb, dtype=torch.int64, device="cuda")
        self.d_offs = torch.zeros(nb, dtype=torch.int64, device="cuda")
        self.d_packed = g("packed", g8, len(self.packed), A5)
        self.cb2 = dict(self.cb, out=g("slots2", g8, nb * c.slot_bytes, A5))
        per = int(c.lib.fsehip_dtable_bytes(c.max_table_log))
        self.tabs = {"dt": g("dt", g32, nb * per // 4, F32), "info": g("dtinfo", g32, nb, F32)}
        self.routes = ["prebuilt tables", "sidecar", "sidecar-less"] + (["build_sidecar"] if self.rebuild else [])
        self.outs = {r: (g(f"{r} out", g8, n, A5), g(f"{r} status", g32, nb, F32)) for r in self.routes}
        if self.rebuild:
            self.side2 = g("sidecar rebuilt", g64, nb * c.side_per_block, F64)
        # what a decoder or the pack reads starts as zeros; pure outputs keep their fill
        self.zeroed = ["slots", "comp_len", "sidecar", "packed", "slots2", "dt"]

    def poison(self):
        self.src.fill_(SRC_POISON)
        for name, (_, view, fill) in self.G.items():
            view.fill_(0 if name in self.zeroed else fill)
        self.len64.zero_()
        self.d_offs.zero_()

    def enqueue(self, step9):
        torch, c, cb, cb2 = self.torch, self.codec, self.cb, self.cb2
        lib, hs = c.lib, stream_ptr(self.torch)
        c.compress_into(self.src, cb)
        # the exclusive scan of comp_len, on this stream
        self.len64.copy_(cb["comp_len"])
        torch.cumsum(self.len64, 0, out=self.d_offs)
        self.d_offs.sub_(self.len64)
        assert lib.fsehip_pack_blocks(ptr(cb["out"]), c.slot_bytes, ptr(cb["comp_len"]), ptr(self.d_offs), self.nb,
                                      ptr(self.d_packed), hs) == 0
        assert lib.fsehip_unpack_blocks(ptr(self.d_packed), ptr(self.d_offs), ptr(cb["comp_len"]), self.nb,
                                        ptr(cb2["out"]), c.slot_bytes, hs) == 0
        c.build_dtables_into(cb2, self.tabs)
        c.decompress_dt_into(cb2, self.tabs, *self.outs["prebuilt tables"])
        c.decompress_into(cb2, *self.outs["sidecar"])
        c.decompress_into(cb2, *self.outs["sidecar-less"], use_sidecar=False)
        if self.rebuild:
            out, st = self.outs["build_sidecar"]
            p = c.params()
            assert lib.fsehip_build_sidecar(C.byref(p), ptr(cb2["out"]), c.slot_bytes, ptr(cb["comp_len"]), ptr(out),
                                            len(self.raw), ptr(self.side2), ptr(st), hs) == 0
        step9()

    def check(self):
        c, cb, nb = self.codec, self.cb, self.nb
        for name, (whole, view, fill) in self.G.items():
            assert_guards(whole, view, fill, name)
        assert cb["status"].tolist() == [0] * nb, cb["status"].tolist()
        same(cb["comp_len"].cpu().numpy(), self.lens, "comp_len")
        same(cb["payload_bits"].cpu().numpy(), [w[1] for w in self.want], "payload_bits")
        for name, slots in (("slots", cb["out"]), ("slots2", self.cb2["out"])):
            host = slots.cpu().numpy()
            for b, w in enumerate(self.want):
                got = host[b * c.slot_bytes: b * c.slot_bytes + len(w[0])].tobytes()
                assert got == w[0], f"{name}: block {b} differs from the oracle"
        same(self.d_offs.cpu().numpy(), self.offs, "offsets")
        same(self.d_packed.cpu().numpy(), self.packed, "packed stream")
        assert bool((self.tabs["info"] >= 0).all()), self.tabs["info"].tolist()
        for route, (out, st) in self.outs.items():
            assert st.tolist() == [0] * nb, (route, st.tolist())
            same(out.cpu().numpy(), self.raw, f"{route} output")
        if self.rebuild:
            spb = c.side_per_block
            got, want = self.side2.cpu().numpy(), cb["sidecar"].cpu().numpy()
            for b, n in enumerate(self.sizes):
                k = valid_checkpoints(n, CKPT, self.nstates)
                same(got[b * spb: b * spb + k], want[b * spb: b * spb + k], f"rebuilt sidecar of block {b}")


# ---------------------------------------------------------------- 2. the frame path
def range_list(n, picks, base=0):
    """single_ranges(n) cases by name as one call's (src_off, len, dst_off)
    list: each destination starts `shift` bytes after a 16-byte boundary."""
    cases = {name: (s, ln, shift) for name, s, ln, shift in single_ranges(n)}
    out, at = [], base
    for name in picks:
        s, ln, shift = cases[name]
        at = (at + 15) // 16 * 16 + shift
        out.append((s, ln, at))
        at += ln + 3
    return out


FRAME_PICKS = ["across one boundary, both partial", "blocks 1..7 whole, aligned: direct",
               "blocks 1..7 whole, destination off by one: bounce", "partial head, direct middle, partial tail",
               "edges in RAW and RLE", "a block's last byte"]


class FrameChain(Chain):
    CHUNK = 3

    def __init__(self, nstates):
        self.nstates = nstates
        self.raw = frame_source(0x5EED0600 + nstates)
        self.frame = R.build_frame(self.raw, BLOCK, CKPT, nstates)
        types = R.types_of(self.frame)
        assert {R.RAW, R.RLE, R.FSE} <= set(types)
        self.non_fse = sum(t != R.FSE for t in types)
        self.ranges = range_list(len(self.raw), FRAME_PICKS)
        self.dst_size = max(d + ln for _, ln, d in self.ranges) + 33
        self.want_dst = expected(self.raw, self.ranges, self.dst_size)

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        self.torch = torch
        c = self.codec = BlockCodec(block_size=BLOCK, ckpt_interval=CKPT, nstates=self.nstates)
        n = len(self.raw)
        self.info = c.frame_info(self.frame)
        assert (self.info.n_total, self.info.n_blocks) == (n, N_BLOCKS + 1)
        self.src = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.uploads = [(self.src, pinned(torch, self.raw))]
        self.w_frame, self.d_frame = g8(torch, c.frame_bound(n))
        self.w_flen, self.flen = g64(torch, 1)
        self.w_cres, self.cres = g32(torch, 2)
        self.w_out, self.out = g8(torch, n)
        self.w_bst, self.bst = g32(torch, self.info.n_blocks)
        self.w_dres, self.dres = g32(torch, 2)
        self.w_dst, self.dst = g8(torch, self.dst_size)
        self.w_rst, self.rst = g32(torch, len(self.ranges))
        self.w_rres, self.rres = g32(torch, 2)
        self.arr = c.frame_ranges(self.ranges)

    def poison(self):
        self.src.fill_(SRC_POISON)
        self.d_frame.zero_()  # what the decoders read: an all-zero frame is BAD_FRAME
        self.flen.fill_(F64)
        for t in (self.out, self.dst):
            t.fill_(A5)
        for t in (self.cres, self.bst, self.dres, self.rst, self.rres):
            t.fill_(F32)

    def enqueue(self, step9):
        c = self.codec
        frame = self.d_frame[: len(self.frame)]  # the expected length: frame_len itself stays on the device
        c.compress_frame_into(self.src, self.d_frame, self.flen, self.cres, chunk_blocks=self.CHUNK)
        c.decompress_frame_into(frame, self.info, self.out, self.bst, self.dres, chunk_blocks=self.CHUNK)
        c.decompress_frame_ranges_into(frame, self.info, self.arr, self.dst, self.rst, self.rres,
                                       chunk_blocks=self.CHUNK)
        step9()

    def check(self):
        for w, v, f, name in ((self.w_frame, self.d_frame, A5, "d_frame"), (self.w_flen, self.flen, F64, "d_frame_len"),
                              (self.w_cres, self.cres, F32, "compress d_result"), (self.w_out, self.out, A5, "d_out"),
                              (self.w_bst, self.bst, F32, "d_block_status"), (self.w_dres, self.dres, F32, "d_result"),
                              (self.w_dst, self.dst, A5, "ranges d_out"), (self.w_rst, self.rst, F32, "d_range_status"),
                              (self.w_rres, self.rres, F32, "ranges d_result")):
            assert_guards(w, v, f, name)
        n = len(self.frame)
        assert self.flen.tolist() == [n], (self.flen.tolist(), n)
        same(self.d_frame[:n].cpu().numpy(), np.frombuffer(self.frame, dtype=np.uint8), "frame bytes")
        assert bool((self.d_frame[n:] == 0).all()), "a store past frame_len"
        assert self.cres.tolist() == [0, self.non_fse], self.cres.tolist()
        assert self.dres.tolist() == [0, 0], self.dres.tolist()
        assert not bool(self.bst.any()), self.bst.tolist()
        same(self.out.cpu().numpy(), self.raw, "frame decode")
        assert self.rres.tolist() == [0, 0], self.rres.tolist()
        assert not bool(self.rst.any()), self.rst.tolist()
        same(self.dst.cpu().numpy(), self.want_dst, "range destination")


# ---------------------------------------------------------------- 3. more range calls than staging buffers
class ManyRangesChain(Chain):
    """20 calls on one frame, each with its own list, destination, statuses
    and result.  The lists differ in their blocks, offsets and lengths but
    share one shape (ranges, pieces, listed and bounce blocks): should a call
    ever run on another call's staged lists, or on a mix of two, every offset
    it then uses is still inside the frame, the scratch and its destination,
    so the failure is wrong bytes and never a stray access.  For the same
    reason a piece that touches a block's end has the same place in its block
    in every call, and every destination has the same size."""
    CALLS = 20
    # (blocks touched, ...) of the five ranges of every call; the blocks of a call's ranges are disjoint
    GROUPS = [2, 1, 4, 2, 2]
    DST = [0, 1344, 3360, 19744, 19776]  # where each range's destination starts (+ 0..15 but for the direct run)
    SIZE = 19776 + 15 + 2 * BLOCK + 33

    def __init__(self):
        self.raw = frame_source(0x5EED0602)
        self.frame = R.build_frame(self.raw, BLOCK, CKPT, 2)
        rng = np.random.default_rng(0x3A9E5)
        B = BLOCK
        self.lists = []
        for i in range(self.CALLS):
            # the five block groups in a random order with random gaps, inside blocks 0..39
            order = rng.permutation(len(self.GROUPS))
            gaps = rng.multinomial(N_BLOCKS - sum(self.GROUPS), np.ones(len(self.GROUPS) + 1) / (len(self.GROUPS) + 1))
            first, at = {}, 0
            for k, g in enumerate(order):
                at += int(gaps[k])
                first[int(g)] = at
                at += self.GROUPS[g]
            assert at <= N_BLOCKS
            j = [int(x) for x in rng.integers(0, 16, 5)]
            self.lists.append([
                (first[0] * B + B - 300, 300 + int(rng.integers(100, 1001)), self.DST[0] + j[0]),  # across a boundary
                (first[1] * B + int(rng.integers(0, 2001)), int(rng.integers(1, 2001)), self.DST[1] + j[1]),  # inside
                (first[2] * B, 4 * B, self.DST[2]),                                   # whole and aligned: direct
                (first[3] * B + B - 1, 2, self.DST[3] + j[3]),                        # a last and a first byte
                (first[4] * B, 2 * B, self.DST[4] + 1 + j[4] % 15),                   # whole, misaligned: bounce
            ])
        assert all(d + ln + 33 <= self.SIZE for r in self.lists for _, ln, d in r)
        assert len({r[2][0] for r in self.lists}) > 5 and len({r[1][1] for r in self.lists}) > 10
        self.want = [expected(self.raw, r, self.SIZE) for r in self.lists]
        self.done_after, self.call_ms = [], []

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        self.torch = torch
        c = self.codec = BlockCodec(block_size=BLOCK, ckpt_interval=CKPT, nstates=2)
        self.info = c.frame_info(self.frame)
        host = np.frombuffer(self.frame, dtype=np.uint8)
        self.d_frame = torch.empty(len(host), dtype=torch.uint8, device="cuda")
        self.uploads = [(self.d_frame, pinned(torch, host))]
        self.bufs = [(g8(torch, self.SIZE), g32(torch, len(r)), g32(torch, 2)) for r in self.lists]
        self.arrs = [c.frame_ranges(r) for r in self.lists]

    def poison(self, inputs=True):
        if inputs:
            self.d_frame.zero_()
        for (_, dst), (_, st), (_, res) in self.bufs:
            dst.fill_(A5)
            st.fill_(F32)
            res.fill_(F32)

    def enqueue(self, step9):
        """Call PIN_BUFS + 1 has to wait for a staging buffer, so for the gate:
        the host must be ahead of the gate after call PIN_BUFS."""
        probe = self.probe
        self.done_after, self.call_ms = [], []
        for i, (arr, ((_, dst), (_, st), (_, res))) in enumerate(zip(self.arrs, self.bufs)):
            t0 = time.perf_counter()
            self.codec.decompress_frame_ranges_into(self.d_frame, self.info, arr, dst, st, res, chunk_blocks=3)
            self.call_ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            if probe is not None:
                self.done_after.append(bool(probe()))
            if i + 1 == PIN_BUFS:
                step9()

    def check(self):
        for i, (((w_d, dst), (w_s, st), (w_r, res)), want) in enumerate(zip(self.bufs, self.want)):
            assert_guards(w_d, dst, A5, f"call {i} d_out")
            assert_guards(w_s, st, F32, f"call {i} d_range_status")
            assert_guards(w_r, res, F32, f"call {i} d_result")
            assert res.tolist() == [0, 0], (i, res.tolist())
            assert not bool(st.any()), (i, st.tolist())
            same(dst.cpu().numpy(), want, f"destination of call {i}")


# ---------------------------------------------------------------- 6. the remaining entry points
class StreamsChain(Chain):
    LENGTHS = [0, 1, 2, 17, 4096, 5000]

    def __init__(self):
        rng = np.random.default_rng(0x57E5)
        alpha = np.array([3, 9, 27, 81, 128, 200, 255], dtype=np.uint8)
        self.raws = []
        for i, n in enumerate(self.LENGTHS):
            raw = O.generate(0, 0.155, 0x5EED0700, i, n) if n >= 64 else alpha[rng.integers(0, 7, n)]
            raw[:2] = [3, 9][:n]  # two symbols at least: the crate encodes it, and its decoder terminates
            self.raws.append(raw)
        self.want = []
        for r in self.raws:
            try:
                self.want.append(O.compress2(r))
            except O.OracleError as e:
                self.want.append(e.code)
        assert self.want[0] == "EMPTY" and self.want[1] == "TOO_SHORT" and not isinstance(self.want[2], str)
        self.out_stride = 5008
        self.back = [w if isinstance(w, str) else O.decompress2(w[0], self.out_stride) for w in self.want]

    def alloc(self, torch):
        from entropy_coders_amd import load
        from entropy_coders_amd._lib import StreamDesc

        self.torch, self.lib = torch, load()
        n = len(self.raws)
        self.stride = (int(self.lib.fsehip_stream_out_bytes(max(self.LENGTHS), 11)) + 255) // 256 * 256
        desc = (StreamDesc * n)()
        so = 0
        for i, r in enumerate(self.raws):
            desc[i] = StreamDesc(so, i * self.stride, len(r), self.stride)  # each region is the decoder's input slot
            so += (len(r) + 15) // 16 * 16
        host = np.zeros(max(so, 16), dtype=np.uint8)
        for i, r in enumerate(self.raws):
            host[desc[i].src_off: desc[i].src_off + len(r)] = r
        hdesc = np.frombuffer(bytes(desc), dtype=np.uint8)
        self.src = torch.empty(len(host), dtype=torch.uint8, device="cuda")
        self.desc = torch.empty(len(hdesc), dtype=torch.uint8, device="cuda")
        self.uploads = [(self.src, pinned(torch, host)), (self.desc, pinned(torch, hdesc))]
        self.w_comp, self.comp = g8(torch, n * self.stride)
        self.w_len, self.comp_len = g32(torch, n)
        self.w_bits, self.bits = g32(torch, n)
        self.w_st, self.st = g32(torch, n)
        self.w_out, self.out = g8(torch, n * self.out_stride)
        self.w_ol, self.out_len = g32(torch, n)
        self.w_dst, self.dst = g32(torch, n)

    def poison(self):
        self.src.fill_(SRC_POISON)
        self.desc.zero_()      # a zero descriptor is an empty stream
        self.comp.zero_()      # the decoder's input
        self.comp_len.zero_()
        self.out.fill_(A5)
        for t in (self.bits, self.st, self.out_len, self.dst):
            t.fill_(F32)

    def enqueue(self, step9):
        n, hs = len(self.raws), stream_ptr(self.torch)
        assert self.lib.fsehip_compress_streams(2, 0, 0, ptr(self.src), ptr(self.desc), n, ptr(self.comp),
                                                ptr(self.comp_len), ptr(self.bits), ptr(self.st), hs) == 0
        assert self.lib.fsehip_decompress_streams(2, 11, ptr(self.comp), self.stride, ptr(self.comp_len), n,
                                                  ptr(self.out), self.out_stride, ptr(self.out_len), ptr(self.dst),
                                                  hs) == 0
        step9()

    def check(self):
        from entropy_coders_amd._lib import STATUS

        for w, v, f, name in ((self.w_comp, self.comp, A5, "d_out"), (self.w_len, self.comp_len, F32, "comp_len"),
                              (self.w_bits, self.bits, F32, "payload_bits"), (self.w_st, self.st, F32, "status"),
                              (self.w_out, self.out, A5, "decode d_out"), (self.w_ol, self.out_len, F32, "out_len"),
                              (self.w_dst, self.dst, F32, "decode status")):
            assert_guards(w, v, f, name)
        comp, out = self.comp.cpu().numpy(), self.out.cpu().numpy()
        cl, pb, st = self.comp_len.tolist(), self.bits.tolist(), self.st.tolist()
        ol, ds = self.out_len.tolist(), self.dst.tolist()
        for i, (w, back) in enumerate(zip(self.want, self.back)):
            if isinstance(w, str):
                assert STATUS[st[i]] == w and cl[i] == 0, (i, w, st[i], cl[i])
                assert ds[i] != 0 and ol[i] == 0, (i, ds[i], ol[i])  # nothing to decode
            else:
                assert st[i] == 0 and cl[i] == len(w[0]) and pb[i] == w[1], (i, st[i], cl[i], pb[i])
                assert comp[i * self.stride: i * self.stride + cl[i]].tobytes() == w[0], i
                assert ds[i] == 0 and ol[i] == len(back), (i, ds[i], ol[i], len(back))
                assert out[i * self.out_stride: i * self.out_stride + ol[i]].tobytes() == back, i
        assert self.back[-1] == self.raws[-1].tobytes()


class CopyChain(Chain):
    def __init__(self):
        rng = np.random.default_rng(0xC0B2)
        lens = rng.permutation(np.array([0, 1, 2, 3, 5, 15, 16, 17, 255, 1021, 4096, 5000] * 2))
        gaps = rng.integers(0, 9, len(lens))
        self.lens = lens.astype(np.int32)
        self.so = (np.cumsum(lens + gaps) - lens).astype(np.int64)
        self.do = (np.cumsum(lens + gaps[::-1]) - lens).astype(np.int64)
        self.n_src, self.n_dst = int(self.so[-1] + lens[-1]) + 3, int(self.do[-1] + lens[-1]) + 5
        self.host = rng.integers(0, 256, self.n_src, dtype=np.uint8)
        self.host[self.host == A5] = 0x5A
        self.want = np.full(self.n_dst, A5, dtype=np.uint8)
        for s, d, n in zip(self.so, self.do, self.lens):
            self.want[d: d + n] = self.host[s: s + n]

    def alloc(self, torch):
        from entropy_coders_amd import load

        self.torch, self.lib = torch, load()
        self.w_src, self.src = g8(torch, self.n_src)  # guarded: whole-dword reads stay inside the allocation
        self.d_so, self.d_do, self.d_ln = (torch.empty(len(self.lens), dtype=dt, device="cuda")
                                           for dt in (torch.int64, torch.int64, torch.int32))
        self.uploads = [(self.src, pinned(torch, self.host)), (self.d_so, pinned(torch, self.so)),
                        (self.d_do, pinned(torch, self.do)), (self.d_ln, pinned(torch, self.lens))]
        self.w_dst, self.dst = g8(torch, self.n_dst)

    def poison(self):
        self.src.fill_(SRC_POISON)
        for t in (self.d_so, self.d_do, self.d_ln):
            t.zero_()  # zero lengths: nothing is copied
        self.dst.fill_(A5)

    def enqueue(self, step9):
        assert self.lib.fsehip_copy_blocks(ptr(self.src), ptr(self.d_so), ptr(self.d_ln), len(self.lens), ptr(self.dst),
                                           ptr(self.d_do), stream_ptr(self.torch)) == 0
        step9()

    def check(self):
        assert_guards(self.w_dst, self.dst, A5, "d_dst")
        same(self.dst.cpu().numpy(), self.want, "copied blocks")


class HistogramChain(Chain):
    def __init__(self):
        self.n = 4 * BLOCK + 15
        rng = np.random.default_rng(0x4158)
        self.host = np.concatenate([O.generate(0, 0.155, 0x5EED0701, 0, 2 * BLOCK),
                                    rng.integers(0, 256, self.n - 2 * BLOCK, dtype=np.uint8)])
        blocks = [self.host[b * BLOCK: (b + 1) * BLOCK] for b in range(5)]
        self.counts = np.concatenate([np.bincount(s, minlength=256) for s in blocks])
        self.table_len = [int(s.max()) + 1 for s in blocks]

    def alloc(self, torch):
        from entropy_coders_amd import load

        self.torch, self.lib = torch, load()
        self.src = torch.empty(self.n + 16, dtype=torch.uint8, device="cuda")
        self.uploads = [(self.src[: self.n], pinned(torch, self.host))]
        self.w_c, self.d_counts = g32(torch, 5 * 256)
        self.w_t, self.d_tl = g32(torch, 5)

    def poison(self):
        self.src.fill_(SRC_POISON)
        self.d_counts.fill_(F32)
        self.d_tl.fill_(F32)

    def enqueue(self, step9):
        assert self.lib.fsehip_histogram_blocks(ptr(self.src), self.n, BLOCK, ptr(self.d_counts), ptr(self.d_tl),
                                                stream_ptr(self.torch)) == 0
        step9()

    def check(self):
        assert_guards(self.w_c, self.d_counts, F32, "d_counts")
        assert_guards(self.w_t, self.d_tl, F32, "d_table_len")
        same(self.d_counts.cpu().numpy(), self.counts, "counts")
        assert self.d_tl.tolist() == self.table_len


class GenerateChain(Chain):
    """fsehip_generate reads no device input: the output is filled on the
    stream behind the gate instead, so a kernel that ran during the gate is
    overwritten by the fill."""
    SEED = 0x5EED0702

    def __init__(self):
        self.n = 3 * BLOCK + 77
        self.want = np.concatenate([O.generate(0, 0.155, self.SEED, b, min(BLOCK, self.n - b * BLOCK))
                                    for b in range(4)])

    def alloc(self, torch):
        from entropy_coders_amd import load

        self.torch, self.lib = torch, load()
        self.w_out, self.out = g8(torch, self.n)

    def poison(self):
        self.out.zero_()

    def upload(self):
        self.out.fill_(A5)

    def enqueue(self, step9):
        assert self.lib.fsehip_generate(0, 0.155, self.SEED, BLOCK, ptr(self.out), self.n,
                                        stream_ptr(self.torch)) == 0
        step9()

    def check(self):
        assert_guards(self.w_out, self.out, A5, "generate d_out")
        same(self.out.cpu().numpy(), self.want, "generated bytes")


class BitsChain(Chain):
    COUNT = 5000  # more than one tile of 4,096 fields

    def __init__(self):
        rng = np.random.default_rng(0xB175 + self.COUNT)
        n = self.COUNT
        self.widths = random_widths(rng, n)
        self.vals = rng.integers(0, 1 << 32, n, dtype=np.uint64)
        self.m = masked(self.vals, self.widths)
        self.stack, wbits = O.bits_write(self.m, self.widths, True)
        self.total = wbits + 1
        self.cap = 4 * ((self.total + 31) // 32)
        got, first, fin = model_stack(np.frombuffer(self.stack, dtype=np.uint8), self.widths[::-1])
        assert first == n and fin and np.array_equal(got, self.m[::-1].astype(np.uint32))
        # a forward stream of its own for the ops reader, overrun by its last read
        self.ops = np.append(rng.integers(0, 3, n), [1, 2, 0]).astype(np.uint8)
        self.rwidths = np.append(random_widths(rng, n), [32, 32, 16]).astype(np.uint8)
        adv = np.minimum(self.rwidths[:n].astype(np.int64), 32)
        adv[self.ops[:n] == 1] = 0
        self.rbits = int(adv.sum()) + 36
        self.rdata = rng.integers(0, 256, (self.rbits + 7) // 8, dtype=np.uint8)
        self.rwant, self.rfirst, fin = model_stream(self.rdata.tobytes(), self.rbits, self.rwidths, self.ops)
        assert self.rfirst == n + 2 and not fin

    def alloc(self, torch):
        from entropy_coders_amd import load

        self.torch, self.lib = torch, load()
        n = self.COUNT

        def dev(a):
            host = pinned(torch, a)
            self.uploads.append((torch.empty_like(host, device="cuda"), host))
            return self.uploads[-1][0]

        self.uploads = []
        self.d_v = dev(np.append(self.vals, 1).astype(np.uint32).view(np.int32))  # unmasked: the writer masks
        self.d_w = dev(np.append(self.widths, 1).astype(np.uint8))                # the last field is the marker bit
        self.d_rw = dev(np.ascontiguousarray(self.widths[::-1]))
        padded = np.zeros((len(self.rdata) + 3) // 4 * 4 + 4, dtype=np.uint8)
        padded[: len(self.rdata)] = self.rdata
        self.d_in = dev(padded)
        self.d_sw, self.d_ops = dev(self.rwidths), dev(self.ops)
        self.inputs = [t for t, _ in self.uploads]
        self.w_o, self.d_out = g8(torch, self.cap)
        self.w_t, self.d_tot = g64(torch, 1)
        self.w_kv, self.k_vals = g32(torch, n)
        self.w_kr, self.k_res = g64(torch, 3)
        self.w_sv, self.s_vals = g32(torch, n + 3)
        self.w_sr, self.s_res = g64(torch, 3)

    def poison(self):
        for t in self.inputs:
            t.zero_()
        self.d_out.zero_()  # the stack reader's input: no marker
        for t in (self.d_tot, self.k_res, self.s_res):
            t.fill_(F64)
        for t in (self.k_vals, self.s_vals):
            t.fill_(F32)

    def enqueue(self, step9):
        lib, hs, n = self.lib, stream_ptr(self.torch), self.COUNT
        assert lib.fsehip_bitstack_write(ptr(self.d_v), ptr(self.d_w), n + 1, ptr(self.d_out), self.cap,
                                         ptr(self.d_tot), hs) == 0
        assert lib.fsehip_bitstack_read(ptr(self.d_out), len(self.stack), ptr(self.d_rw), n, ptr(self.k_vals),
                                        ptr(self.k_res), hs) == 0
        assert lib.fsehip_bitstream_read_ops(ptr(self.d_in), len(self.rdata), self.rbits, ptr(self.d_sw),
                                             ptr(self.d_ops), n + 3, ptr(self.s_vals), ptr(self.s_res), hs) == 0
        step9()

    def check(self):
        for w, v, f, name in ((self.w_o, self.d_out, A5, "d_out"), (self.w_t, self.d_tot, F64, "d_total_bits"),
                              (self.w_kv, self.k_vals, F32, "stack d_vals"), (self.w_kr, self.k_res, F64, "stack d_result"),
                              (self.w_sv, self.s_vals, F32, "stream d_vals"),
                              (self.w_sr, self.s_res, F64, "stream d_result")):
            assert_guards(w, v, f, name)
        assert self.d_tot.tolist() == [self.total]
        assert self.d_out[: len(self.stack)].cpu().numpy().tobytes() == self.stack
        assert self.k_res.tolist() == [self.COUNT, 1, 0], self.k_res.tolist()
        same(self.k_vals.cpu().numpy().view(np.uint32), self.m[::-1].astype(np.uint32), "stack reads")
        assert self.s_res.tolist() == [self.rfirst, 0, 0], self.s_res.tolist()
        same(self.s_vals.cpu().numpy().view(np.uint32)[: self.rfirst], self.rwant, "stream steps")


BLOCK_PARAMS = [(2, 0, 4096, N_BLOCKS), (1, 0, 4096, N_BLOCKS), (2, 13, 1024, N_BLOCKS), (2, 0, 1024, 300)]
CHAINS = {f"blocks-{ns}s-L{L}-{bs}x{nb}": (lambda ns=ns, L=L, bs=bs, nb=nb: BlockChain(ns, L, bs, nb, L != 13))
          for ns, L, bs, nb in BLOCK_PARAMS}
CHAINS.update({"frame-2s": lambda: FrameChain(2), "frame-1s": lambda: FrameChain(1), "ranges-x20": ManyRangesChain,
               "streams": StreamsChain, "copy_blocks": CopyChain, "histogram_blocks": HistogramChain,
               "generate": GenerateChain, "bits": BitsChain})


def test_host_side_of_the_chains():
    """No GPU: the host side of every chain builds, with the oracle's results and the models' own checks."""
    for make in CHAINS.values():
        make()


# ---------------------------------------------------------------- the gate
class Ctx:
    def __init__(self, torch):
        self.torch = torch
        self.S = torch.cuda.Stream()
        self.enqueue_ms, self.failed, self.chains = {}, {}, {}
        self.gate_ms = GATE_CAP_MS
        # cycles of torch.cuda._sleep per millisecond, timed with events
        cycles = 20_000_000
        with torch.cuda.stream(self.S):
            torch.cuda._sleep(1_000_000)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
        self.S.synchronize()
        self.cycles_per_ms = cycles / max(e0.elapsed_time(e1), 1e-3)

    def gate(self, ms=None):
        """A bounded spin of `ms` on the current stream, then the event that marks its end."""
        left = int((ms or self.gate_ms) * self.cycles_per_ms)
        while left > 0:
            self.torch.cuda._sleep(min(left, 1 << 30))
            left -= 1 << 30
        done = self.torch.cuda.Event()
        done.record()
        return done

    def run(self, chain, gated, stream=None):
        """Steps 3..10 for one chain.  Returns the host time of the enqueue up to step 9 in ms."""
        torch, S = self.torch, stream or self.S
        if gated:
            # the chain once on the poison alone: whatever the workspace still held of the warm-up pass (the same
            # data, so the right answers) is now what the poison gives, failure statuses mostly
            chain.poison()
            torch.cuda.synchronize()
            chain.probe = None
            with torch.cuda.stream(S):
                chain.enqueue(lambda: None)
            S.synchronize()
        chain.poison()
        torch.cuda.synchronize()
        mark = {}
        with torch.cuda.stream(S):
            gate_done = self.gate() if gated else None

            def step9():
                mark["t"] = time.perf_counter()
                mark["behind"] = gate_done is None or not gate_done.query()

            chain.upload()
            t0 = time.perf_counter()
            chain.probe = gate_done.query if gated else None
            chain.enqueue(step9)
        assert "t" in mark, "the chain never reached step 9"
        ms = (mark["t"] - t0) * 1e3
        if gated:
            assert mark["behind"], (f"the gate of {self.gate_ms:.1f} ms had passed when the calls returned after "
                                    f"{ms:.2f} ms: some call waited for the stream"
                                    + (f"; ms per call {chain.call_ms}" if hasattr(chain, "call_ms") else ""))
        S.synchronize()
        chain.check()
        return ms


@pytest.fixture(scope="module")
def warm(torch_cuda):
    """Every chain once, ungated, on S: results checked, workspaces grown,
    enqueue times measured; then the gate length."""
    ctx = Ctx(torch_cuda)
    for name, make in CHAINS.items():
        try:
            chain = make()
            chain.alloc(torch_cuda)
            ctx.chains[name] = chain
            ctx.run(chain, gated=False)                        # the first call of a kernel loads its code
            ctx.enqueue_ms[name] = ctx.run(chain, gated=False)
        except Exception as e:  # reported by that chain's own test
            torch_cuda.cuda.synchronize()
            ctx.failed[name] = e
    longest = max(ctx.enqueue_ms.values(), default=GATE_CAP_MS)
    ctx.gate_ms = min(GATE_CAP_MS, max(GATE_FACTOR * longest, GATE_FLOOR_MS))
    print(f"\n[stream order] enqueue ms: " + ", ".join(f"{k} {v:.2f}" for k, v in ctx.enqueue_ms.items()))
    print(f"[stream order] longest enqueue {longest:.2f} ms, gate {ctx.gate_ms:.1f} ms "
          f"({ctx.cycles_per_ms:.0f} sleep cycles per ms)")
    return ctx


def behind_gate(warm, name):
    if name in warm.failed:
        raise warm.failed[name]
    ms = warm.run(warm.chains[name], gated=True)
    print(f"\n[stream order] {name}: enqueue {ms:.2f} ms behind a gate of {warm.gate_ms:.1f} ms "
          f"(ungated {warm.enqueue_ms[name]:.2f} ms)")
    return warm.chains[name]


@gpu
@pytest.mark.parametrize("name", [k for k in CHAINS if k.startswith("blocks")])
def test_block_path_one_chain(warm, name):
    behind_gate(warm, name)


@gpu
@pytest.mark.parametrize("name", ["frame-2s", "frame-1s"])
def test_frame_path_one_chain(warm, name):
    behind_gate(warm, name)


@gpu
def test_more_range_calls_than_staging_buffers(warm):
    """20 calls behind one gate: the first 8 return at once (step 9 comes
    after the 8th), the 9th waits for the oldest buffer's copy, that is for
    the gate; then all 20 again, ungated, on buffers whose events have passed."""
    chain = behind_gate(warm, "ranges-x20")
    print(f"[stream order] gate passed after call: {chain.done_after}")
    assert not any(chain.done_after[:PIN_BUFS]), chain.done_after
    chain.probe = None
    chain.poison(inputs=False)
    warm.torch.cuda.synchronize()
    with warm.torch.cuda.stream(warm.S):
        chain.enqueue(lambda: None)
    warm.S.synchronize()
    chain.check()


@gpu
@pytest.mark.parametrize("name", ["streams", "copy_blocks", "histogram_blocks", "generate", "bits"])
def test_remaining_entry_points(warm, name):
    behind_gate(warm, name)


# ---------------------------------------------------------------- 4. workspace growth behind pending work
class DecodeBatch:
    """Oracle-compressed blocks as slots on the device: a sidecar-less decode's input."""

    def __init__(self, torch, codec, seed, n_blocks):
        blocks = lut_blocks(seed, BLOCK, n_blocks, TAIL)
        self.raw = np.concatenate(blocks)
        slots, lens = host_slots([O.compress2(s)[0] for s in blocks], codec.slot_bytes)
        self.h_slots, self.h_lens = pinned(torch, slots), pinned(torch, lens)
        nb = len(blocks)
        self.cb = {"n_total": len(self.raw), "out": torch.zeros(len(slots), dtype=torch.uint8, device="cuda"),
                   "comp_len": torch.zeros(nb, dtype=torch.int32, device="cuda"), "sidecar": None}
        self.nb = nb

    def upload(self):
        self.cb["out"].copy_(self.h_slots, non_blocking=True)
        self.cb["comp_len"].copy_(self.h_lens, non_blocking=True)

    def outputs(self, torch):
        return g8(torch, len(self.raw)), g32(torch, self.nb)


@gpu
def test_workspace_growth_behind_pending_work(warm):
    """A small batch, at once a large one (tables, states and bulk scratch
    grow: the old buffers are freed after a synchronise), the small one again.
    The growth waits, so there is no step 9 here: the outputs decide."""
    torch = warm.torch
    from entropy_coders_amd import BlockCodec

    codec = BlockCodec(block_size=BLOCK, ckpt_interval=0, nstates=2)
    S = torch.cuda.Stream()
    small, big = DecodeBatch(torch, codec, 0x5EED0800, 3), DecodeBatch(torch, codec, 0x5EED0801, 63)
    f_small, f_big = frame_source(0x5EED0802, 3), frame_source(0x5EED0803, 63)
    frames = [R.build_frame(r, BLOCK, CKPT, 2) for r in (f_small, f_big)]
    infos = [codec.frame_info(f) for f in frames]
    h_frames = [pinned(torch, np.frombuffer(f, dtype=np.uint8)) for f in frames]
    d_frames = [torch.zeros(len(f), dtype=torch.uint8, device="cuda") for f in frames]
    runs = [(b, b.outputs(torch)) for b in (small, big, small)]
    f_outs = [(g8(torch, len(r)), g32(torch, i.n_blocks), g32(torch, 2)) for r, i in zip((f_small, f_big), infos)]
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        codec.release_workspace()
        warm.gate()
        small.upload()
        big.upload()
        for d, h in zip(d_frames, h_frames):
            d.copy_(h, non_blocking=True)
        for batch, ((_, out), (_, st)) in runs:
            codec.decompress_into(batch.cb, out, st, use_sidecar=False)
        for d, info, ((_, out), (_, st), (_, res)) in zip(d_frames, infos, f_outs):
            codec.decompress_frame_into(d, info, out, st, res)
    S.synchronize()
    for i, (batch, ((w_o, out), (w_s, st))) in enumerate(runs):
        assert_guards(w_o, out, A5, f"decode {i} out")
        assert_guards(w_s, st, F32, f"decode {i} status")
        assert st.tolist() == [0] * batch.nb, (i, st.tolist())
        same(out.cpu().numpy(), batch.raw, f"decode {i} ({batch.nb} blocks)")
    for i, (raw, ((w_o, out), (w_s, st), (w_r, res))) in enumerate(zip((f_small, f_big), f_outs)):
        assert_guards(w_o, out, A5, f"frame {i} out")
        assert_guards(w_s, st, F32, f"frame {i} block status")
        assert_guards(w_r, res, F32, f"frame {i} result")
        assert res.tolist() == [0, 0] and not bool(st.any()), (i, res.tolist(), st.tolist())
        same(out.cpu().numpy(), raw, f"frame {i} decode")
    with torch.cuda.stream(S):
        codec.release_workspace()


# ---------------------------------------------------------------- 5. two streams, two workspaces
class RoundTrip(Chain):
    """compress_into + sidecar-less decompress_into + a frame round trip of one source."""

    def __init__(self, seed):
        self.raw = frame_source(seed, 8)
        blocks = [self.raw[b * BLOCK: (b + 1) * BLOCK] for b in range(9)]
        self.comp = []
        for s in blocks:  # the all-zero block has no FSE form: its status says so
            try:
                self.comp.append(O.compress2(s)[0])
            except O.OracleError as e:
                self.comp.append(e.code)
        assert [c for c in self.comp if isinstance(c, str)] == ["ALL_ZERO_SYMBOL0"]
        self.frame = R.build_frame(self.raw, BLOCK, CKPT, 2)

    def alloc(self, torch):
        from entropy_coders_amd import BlockCodec

        self.torch = torch
        c = self.codec = BlockCodec(block_size=BLOCK, ckpt_interval=CKPT, nstates=2)
        n, nb = len(self.raw), 9
        self.info = c.frame_info(self.frame)
        self.src = torch.empty(n, dtype=torch.uint8, device="cuda")
        self.uploads = [(self.src, pinned(torch, self.raw))]
        self.cb = c.alloc(n)
        self.w_out, self.out = g8(torch, n)
        self.st = torch.empty(nb, dtype=torch.int32, device="cuda")
        self.w_frame, self.d_frame = g8(torch, c.frame_bound(n))
        self.flen = torch.empty(1, dtype=torch.int64, device="cuda")
        self.cres, self.dres, self.bst = (torch.empty(k, dtype=torch.int32, device="cuda") for k in (2, 2, nb))
        self.w_fout, self.fout = g8(torch, n)

    def poison(self):
        self.src.fill_(SRC_POISON)
        for t in (self.cb["out"], self.cb["comp_len"], self.cb["sidecar"], self.d_frame):
            t.zero_()
        for t in (self.out, self.fout):
            t.fill_(A5)
        self.flen.fill_(F64)
        for t in (self.cb["status"], self.cb["payload_bits"], self.st, self.cres, self.dres, self.bst):
            t.fill_(F32)

    def enqueue(self, step9):
        c = self.codec
        c.compress_into(self.src, self.cb)
        c.decompress_into(self.cb, self.out, self.st, use_sidecar=False)
        c.compress_frame_into(self.src, self.d_frame, self.flen, self.cres)
        c.decompress_frame_into(self.d_frame[: len(self.frame)], self.info, self.fout, self.bst, self.dres)
        step9()

    def check(self):
        from entropy_coders_amd._lib import STATUS

        c = self.codec
        for w, v, name in ((self.w_out, self.out, "out"), (self.w_frame, self.d_frame, "d_frame"),
                           (self.w_fout, self.fout, "frame out")):
            assert_guards(w, v, A5, name)
        slots, cl = self.cb["out"].cpu().numpy(), self.cb["comp_len"].tolist()
        est, dst, got = self.cb["status"].tolist(), self.st.tolist(), self.out.cpu().numpy()
        for b, w in enumerate(self.comp):
            lo = b * BLOCK
            if isinstance(w, str):
                assert STATUS[est[b]] == w and cl[b] == 0 and dst[b] != 0, (b, est[b], cl[b], dst[b])
            else:
                assert est[b] == 0 and slots[b * c.slot_bytes: b * c.slot_bytes + cl[b]].tobytes() == w, b
                assert dst[b] == 0, (b, dst[b])
                same(got[lo: lo + BLOCK], self.raw[lo: lo + BLOCK], f"block {b}")
        n = len(self.frame)
        assert self.flen.tolist() == [n]
        same(self.d_frame[:n].cpu().numpy(), np.frombuffer(self.frame, dtype=np.uint8), "frame bytes")
        assert self.cres.tolist()[0] == 0 and self.dres.tolist() == [0, 0] and not bool(self.bst.any())
        same(self.fout.cpu().numpy(), self.raw, "frame decode")


def streams_side_by_side(warm):
    """Two fresh streams of which the second runs while the first is held: a
    process has few hardware queues, and two streams that share one run in
    turn whatever the library does."""
    torch = warm.torch
    S1 = torch.cuda.Stream()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for _ in range(8):
        S2 = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(S1):
            held = warm.gate(20.0)
        with torch.cuda.stream(S2):
            flag.fill_(1)
            ran = torch.cuda.Event()
            ran.record()
        ran.synchronize()
        beside = not held.query()
        S1.synchronize()
        if beside:
            return S1, S2
    pytest.fail("no second stream ran beside a held one: the case cannot be made")


@gpu
def test_two_streams_two_workspaces(warm):
    """S1 is gated, S2 is not: S2's calls run to their end while S1's wait, on
    workspaces of their own.  Were the scratch keyed by the device alone, S2's
    tables and slots would replace S1's before S1's kernels ran."""
    torch = warm.torch
    S1, S2 = streams_side_by_side(warm)
    a, b = RoundTrip(0x5EED0900), RoundTrip(0x5EED0901)
    a.alloc(torch)
    b.alloc(torch)
    warm.run(a, gated=False, stream=S1)  # the workspaces of both streams exist and have their size
    warm.run(b, gated=False, stream=S2)
    a.poison()
    b.poison()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(S1):
        gate_done = warm.gate()
        a.upload()
        a.enqueue(lambda: None)
    with torch.cuda.stream(S2):
        b.upload()
        b.enqueue(lambda: None)
    t1 = time.perf_counter()
    assert not gate_done.query(), f"the calls returned after {(t1 - t0) * 1e3:.2f} ms: some call waited for a stream"
    S2.synchronize()
    t2 = time.perf_counter()
    print(f"\n[stream order] two streams: enqueue {(t1 - t0) * 1e3:.2f} ms, S2 done after {(t2 - t0) * 1e3:.2f} ms, "
          f"gate {warm.gate_ms:.1f} ms")
    assert not gate_done.query(), "S2 ended only after S1's gate: its work did not run beside S1's"
    b.check()
    S1.synchronize()
    a.check()
    for S in (S1, S2):
        with torch.cuda.stream(S):
            a.codec.release_workspace()
    warm.run(a, gated=False, stream=S1)
