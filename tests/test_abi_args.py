"""Argument checks of the C ABI, one row per distinct check plus the pairs
whose precedence matters: a table of malformed (or empty) calls with the
status each returns.

Every row is decided before the library asks for a device, so the expected
status is never NO_DEVICE or HIP and no row runs device work: the fake
non-null pointers (as in test_abi.py) are never dereferenced, with or
without a GPU.  A call whose rejection comes after the device check (the
alignment checks of fsehip_decompress_blocks, the per-buffer statuses of
fse_compress*_many) does not belong here."""
import ctypes as C

import pytest

from entropy_coders_amd import _lib

OK = C.c_void_p(4096)          # a well-aligned fake device or host pointer
ODD = C.c_void_p(4096 + 8)     # off by 8
ODD2 = C.c_void_p(4096 + 2)    # off by 2
SLOT = 90880                   # a multiple of 256
BIG = 1 << 29                  # a block above the 2^28 limit


def params(block=65536, table_log=0, ckpt=0, mtl=11, nstates=2):
    return C.byref(_lib.Params(block, table_log, ckpt, mtl, nstates))


def fparams(block=65536, table_log=0, ckpt=0, mtl=11, nstates=2, chunk=0):
    return C.byref(_lib.FrameParams(block, table_log, ckpt, mtl, nstates, chunk))


def info(n_total=100000, n_blocks=2, block=65536, nstates=2, mtl=11, flags=0, ckpt=0):
    return C.byref(_lib.FrameInfo(1, nstates, mtl, flags, block, ckpt, n_blocks, 0, n_total, 0))


def ranges(*r):
    return (_lib.FrameRange * len(r))(*[_lib.FrameRange(*x) for x in r])


def size(v=0):
    return C.byref(C.c_size_t(v))


ROWS = []


def row(name, want, call):
    ROWS.append(pytest.param(call, want, id=name))


# fsehip_compress_blocks(p, d_src, n_total, d_out, slot_bytes, d_comp_len, d_payload_bits, d_sidecar, d_status, stream)
def cb(p=None, src=OK, n=65536, out=OK, slot=SLOT, clen=OK, side=None, status=OK):
    p = params() if p is None else p
    return lambda lib: lib.fsehip_compress_blocks(p, src, n, out, slot, clen, OK, side, status, None)


row("compress_blocks-null-p", "BAD_ARG", lambda lib: lib.fsehip_compress_blocks(None, OK, 65536, OK, SLOT, OK, OK, None, OK, None))
row("compress_blocks-null-src", "BAD_ARG", cb(src=None))
row("compress_blocks-null-out", "BAD_ARG", cb(out=None))
row("compress_blocks-null-comp_len", "BAD_ARG", cb(clen=None))
row("compress_blocks-null-status", "BAD_ARG", cb(status=None))
row("compress_blocks-empty", "EMPTY", cb(n=0))
row("compress_blocks-empty-before-block-limit", "EMPTY", cb(p=params(block=BIG), n=0))
row("compress_blocks-block-limit", "UNSUPPORTED", cb(p=params(block=BIG), n=BIG))
row("compress_blocks-block-limit-before-nstates", "UNSUPPORTED", cb(p=params(block=BIG, nstates=3), n=BIG))
row("compress_blocks-two-blocks-of-1000", "BAD_ARG", cb(p=params(block=1000), n=2000))
row("compress_blocks-slot-90888", "BAD_ARG", cb(slot=90888))
row("compress_blocks-nstates-3", "BAD_ARG", cb(p=params(nstates=3)))
for side in (None, OK):
    tag = "sidecar" if side else "no-sidecar"
    row(f"compress_blocks-interval-4-{tag}", "BAD_ARG", cb(p=params(ckpt=4), side=side))
    row(f"compress_blocks-interval-8-one-state-{tag}", "BAD_ARG", cb(p=params(ckpt=8, nstates=1), side=side))
    row(f"compress_blocks-interval-24-{tag}", "BAD_ARG", cb(p=params(ckpt=24), side=side))


# fsehip_decompress_blocks_dt(p, d_in, slot, d_comp_len, d_sidecar, d_dtables, d_dtinfo, d_out, n_total, d_status, stream)
def dt(p=None, d_in=OK, slot=SLOT, side=None, tab=OK, tinfo=OK, out=OK, n=65536):
    p = params(mtl=12) if p is None else p
    return lambda lib: lib.fsehip_decompress_blocks_dt(p, d_in, slot, OK, side, tab, tinfo, out, n, OK, None)


row("decompress_blocks_dt-empty", "EMPTY", dt(n=0))
row("decompress_blocks_dt-empty-before-null-tables", "EMPTY", dt(n=0, tab=None))
row("decompress_blocks_dt-null-tables", "BAD_ARG", dt(tab=None))
row("decompress_blocks_dt-null-table-info", "BAD_ARG", dt(tinfo=None))
row("decompress_blocks_dt-null-p", "BAD_ARG", lambda lib: lib.fsehip_decompress_blocks_dt(None, OK, SLOT, OK, None, OK, OK, OK, 65536, OK, None))
row("decompress_blocks_dt-sidecar-interval-0", "BAD_ARG", dt(side=OK))
row("decompress_blocks_dt-sidecar-interval-24", "BAD_ARG", dt(p=params(ckpt=24, mtl=12), side=OK))
row("decompress_blocks_dt-sidecar-interval-8-one-state", "BAD_ARG", dt(p=params(ckpt=8, mtl=12, nstates=1), side=OK))
row("decompress_blocks_dt-slot-not-32", "BAD_ARG", dt(slot=SLOT + 16))
row("decompress_blocks_dt-in-misaligned", "BAD_ARG", dt(d_in=ODD))
row("decompress_blocks_dt-out-misaligned", "BAD_ARG", dt(out=ODD))
row("decompress_blocks_dt-block-limit", "UNSUPPORTED", dt(p=params(block=BIG, mtl=12), n=BIG))
row("decompress_blocks_dt-block-limit-before-alignment", "UNSUPPORTED", dt(p=params(block=BIG, mtl=12), n=BIG, out=ODD))
row("decompress_blocks_dt-two-blocks-of-1000", "BAD_ARG", dt(p=params(block=1000, mtl=12), n=2000))
row("decompress_blocks_dt-nstates-3", "BAD_ARG", dt(p=params(mtl=12, nstates=3)))


# fsehip_decompress_blocks(p, d_in, slot, d_comp_len, d_sidecar, d_out, n_total, d_status, stream)
def db(p=None, side=None, n=65536):
    p = params() if p is None else p
    return lambda lib: lib.fsehip_decompress_blocks(p, OK, SLOT, OK, side, OK, n, OK, None)


row("decompress_blocks-empty", "EMPTY", db(n=0))
row("decompress_blocks-null-p", "BAD_ARG", lambda lib: lib.fsehip_decompress_blocks(None, OK, SLOT, OK, None, OK, 65536, OK, None))
row("decompress_blocks-sidecar-interval-0", "BAD_ARG", db(side=OK))
row("decompress_blocks-block-limit", "UNSUPPORTED", db(p=params(block=BIG), n=BIG))


# fsehip_build_sidecar(p, d_in, slot, d_comp_len, d_out, n_total, d_sidecar_out, d_status, stream)
def bs(p=None, n=65536, side=OK):
    p = params(ckpt=128) if p is None else p
    return lambda lib: lib.fsehip_build_sidecar(p, OK, SLOT, OK, OK, n, side, OK, None)


row("build_sidecar-empty", "EMPTY", bs(n=0))
row("build_sidecar-null-sidecar_out", "BAD_ARG", bs(side=None))
row("build_sidecar-one-state-log-13", "UNSUPPORTED", bs(p=params(ckpt=128, mtl=13, nstates=1)))
row("build_sidecar-one-state-log-13-before-interval", "UNSUPPORTED", bs(p=params(ckpt=24, mtl=13, nstates=1)))
row("build_sidecar-interval-24", "BAD_ARG", bs(p=params(ckpt=24)))
row("build_sidecar-interval-8-one-state", "BAD_ARG", bs(p=params(ckpt=8, nstates=1)))
row("build_sidecar-interval-before-block-limit", "BAD_ARG", bs(p=params(block=BIG, ckpt=24), n=BIG))
row("build_sidecar-block-limit", "UNSUPPORTED", bs(p=params(block=BIG, ckpt=128), n=BIG))

# fsehip_build_dtables(p, d_in, slot, d_comp_len, n_blocks, d_dtables, d_dtinfo, stream)
row("build_dtables-slot-128", "BAD_ARG", lambda lib: lib.fsehip_build_dtables(params(), OK, 128, OK, 4, OK, OK, None))
row("build_dtables-null-tables", "BAD_ARG", lambda lib: lib.fsehip_build_dtables(params(), OK, SLOT, OK, 4, None, OK, None))
row("build_dtables-no-blocks", "OK", lambda lib: lib.fsehip_build_dtables(params(), OK, SLOT, OK, 0, OK, OK, None))
row("build_dtables-slot-128-before-no-blocks", "BAD_ARG", lambda lib: lib.fsehip_build_dtables(params(), OK, 128, OK, 0, OK, OK, None))


# fsehip_compress_streams(nstates, table_log, mtl, d_src, d_desc, n_streams, d_out, d_comp_len, d_payload_bits, d_status, stream)
def cs(nstates=2, mtl=11, src=OK, n=4, out=OK):
    return lambda lib: lib.fsehip_compress_streams(nstates, 0, mtl, src, OK, n, out, OK, OK, OK, None)


row("compress_streams-no-streams", "OK", cs(n=0))
row("compress_streams-no-streams-before-nstates", "OK", cs(n=0, nstates=3))
row("compress_streams-nstates-3", "BAD_ARG", cs(nstates=3))
row("compress_streams-src-misaligned", "BAD_ARG", cs(src=ODD))
row("compress_streams-out-misaligned", "BAD_ARG", cs(out=ODD))
row("compress_streams-too-many", "UNSUPPORTED", cs(n=(1 << 24) + 1))
row("compress_streams-log-16", "UNSUPPORTED", cs(mtl=16))
row("compress_streams-nstates-before-log-16", "BAD_ARG", cs(nstates=3, mtl=16))


# fsehip_decompress_streams(nstates, mtl, d_in, in_stride, d_comp_len, n_streams, d_out, out_stride, d_out_len, d_status, stream)
def ds(mtl=11, in_stride=256, n=4, out=OK, out_stride=24000):
    return lambda lib: lib.fsehip_decompress_streams(2, mtl, OK, in_stride, OK, n, out, out_stride, OK, OK, None)


row("decompress_streams-no-streams", "EMPTY", ds(n=0))
row("decompress_streams-out_stride-0", "BAD_ARG", ds(out_stride=0))
row("decompress_streams-in_stride-128", "BAD_ARG", ds(in_stride=128))
row("decompress_streams-out_stride-24008", "BAD_ARG", ds(out_stride=24008))
row("decompress_streams-out-misaligned", "BAD_ARG", ds(out=ODD))
row("decompress_streams-log-16", "UNSUPPORTED", ds(mtl=16))
row("decompress_streams-alignment-before-log-16", "BAD_ARG", ds(mtl=16, out=ODD))

# fsehip_pack_blocks(d_slots, slot_bytes, d_comp_len, d_offsets, n_blocks, d_stream, stream)
# fsehip_unpack_blocks(d_stream, d_offsets, d_comp_len, n_blocks, d_slots, slot_bytes, stream)
# fsehip_copy_blocks(d_src, d_src_offsets, d_lens, n_blocks, d_dst, d_dst_offsets, stream)
row("pack_blocks-null-stream", "BAD_ARG", lambda lib: lib.fsehip_pack_blocks(OK, SLOT, OK, OK, 4, None, None))
row("pack_blocks-slot-8", "BAD_ARG", lambda lib: lib.fsehip_pack_blocks(OK, 8, OK, OK, 4, OK, None))
row("pack_blocks-no-blocks", "OK", lambda lib: lib.fsehip_pack_blocks(OK, SLOT, OK, OK, 0, OK, None))
row("pack_blocks-null-before-no-blocks", "BAD_ARG", lambda lib: lib.fsehip_pack_blocks(None, SLOT, OK, OK, 0, OK, None))
row("unpack_blocks-null-slots", "BAD_ARG", lambda lib: lib.fsehip_unpack_blocks(OK, OK, OK, 4, None, SLOT, None))
row("unpack_blocks-slot-8", "BAD_ARG", lambda lib: lib.fsehip_unpack_blocks(OK, OK, OK, 4, OK, 8, None))
row("unpack_blocks-no-blocks", "OK", lambda lib: lib.fsehip_unpack_blocks(OK, OK, OK, 0, OK, SLOT, None))
row("unpack_blocks-null-before-no-blocks", "BAD_ARG", lambda lib: lib.fsehip_unpack_blocks(None, OK, OK, 0, OK, SLOT, None))
row("copy_blocks-null-lens", "BAD_ARG", lambda lib: lib.fsehip_copy_blocks(OK, OK, None, 4, OK, OK, None))
row("copy_blocks-no-blocks", "OK", lambda lib: lib.fsehip_copy_blocks(OK, OK, OK, 0, OK, OK, None))
row("copy_blocks-no-blocks-before-null", "OK", lambda lib: lib.fsehip_copy_blocks(None, OK, OK, 0, OK, OK, None))

# fsehip_histogram_blocks(d_src, n_total, block_size, d_counts, d_table_len, stream)
row("histogram_blocks-null-counts", "BAD_ARG", lambda lib: lib.fsehip_histogram_blocks(OK, 65536, 65536, None, OK, None))
row("histogram_blocks-null-src", "BAD_ARG", lambda lib: lib.fsehip_histogram_blocks(None, 65536, 65536, OK, OK, None))
row("histogram_blocks-two-blocks-of-1000", "BAD_ARG", lambda lib: lib.fsehip_histogram_blocks(OK, 2000, 1000, OK, OK, None))

# fsehip_generate(kind, prob, seed, block_size, d_out, n_total, stream)
row("generate-kind-3", "BAD_ARG", lambda lib: lib.fsehip_generate(3, 0.2, 1, 65536, OK, 65536, None))
row("generate-null-out", "BAD_ARG", lambda lib: lib.fsehip_generate(0, 0.2, 1, 65536, None, 65536, None))
row("generate-nothing", "OK", lambda lib: lib.fsehip_generate(0, 0.2, 1, 65536, OK, 0, None))
row("generate-kind-3-before-nothing", "BAD_ARG", lambda lib: lib.fsehip_generate(3, 0.2, 1, 65536, OK, 0, None))


# fsehip_frame_compress(p, d_src, n_total, d_frame, frame_cap, d_frame_len, d_result, stream)
def fc(p=None, src=OK, n=100000, cap=1 << 20, result=OK):
    p = fparams() if p is None else p
    return lambda lib: lib.fsehip_frame_compress(p, src, n, OK, cap, OK, result, None)


row("frame_compress-null-result", "BAD_ARG", fc(result=None))
row("frame_compress-null-src", "BAD_ARG", fc(src=None))
row("frame_compress-block-limit", "UNSUPPORTED", fc(p=fparams(block=BIG), n=BIG, cap=1 << 40))
row("frame_compress-block-limit-before-nstates", "UNSUPPORTED", fc(p=fparams(block=BIG, nstates=3), n=BIG, cap=1 << 40))
row("frame_compress-two-blocks-of-1000", "BAD_ARG", fc(p=fparams(block=1000), n=2000))
row("frame_compress-nstates-3", "BAD_ARG", fc(p=fparams(nstates=3)))
row("frame_compress-src-misaligned", "BAD_ARG", fc(src=ODD))
row("frame_compress-interval-24", "BAD_ARG", fc(p=fparams(ckpt=24)))
row("frame_compress-interval-8-one-state", "BAD_ARG", fc(p=fparams(ckpt=8, nstates=1)))
row("frame_compress-interval-before-frame_cap", "BAD_ARG", fc(p=fparams(ckpt=24), cap=0))
row("frame_compress-frame_cap-one-short", "DST_TOO_SMALL",
    lambda lib: lib.fsehip_frame_compress(fparams(), OK, 100000, OK, lib.fsehip_frame_bound(100000, 65536) - 1, OK, OK, None))


# fsehip_frame_decompress(info, chunk_blocks, d_frame, frame_len, d_out, out_cap, d_block_status, d_result, stream)
def fd(i=None, out=OK, cap=100000, result=OK):
    i = info() if i is None else i
    return lambda lib: lib.fsehip_frame_decompress(i, 0, OK, 1 << 20, out, cap, OK, result, None)


row("frame_decompress-null-info", "BAD_ARG", lambda lib: lib.fsehip_frame_decompress(None, 0, OK, 1 << 20, OK, 100000, OK, OK, None))
row("frame_decompress-null-result", "BAD_ARG", fd(result=None))
row("frame_decompress-n_blocks-wrong", "BAD_ARG", fd(i=info(n_blocks=3)))
row("frame_decompress-block-limit", "UNSUPPORTED", fd(i=info(block=BIG, n_total=BIG, n_blocks=1), cap=BIG))
row("frame_decompress-out-misaligned", "BAD_ARG", fd(out=ODD))
row("frame_decompress-out_cap-one-short", "DST_TOO_SMALL", fd(cap=99999))
row("frame_decompress-alignment-before-out_cap", "BAD_ARG", fd(out=ODD, cap=99999))


# fsehip_frame_decompress_ranges(info, chunk_blocks, d_frame, frame_len, ranges, n_ranges, d_out, out_cap,
#                                d_range_status, d_result, stream)
def fr(r, n_ranges=1, i=None, cap=100000, out=OK):
    i = info() if i is None else i
    return lambda lib: lib.fsehip_frame_decompress_ranges(i, 0, OK, 1 << 20, r, n_ranges, out, cap, OK, OK, None)


row("frame_ranges-null-ranges", "BAD_ARG", fr(None))
row("frame_ranges-null-info", "BAD_ARG",
    lambda lib: lib.fsehip_frame_decompress_ranges(None, 0, OK, 1 << 20, ranges((0, 16, 0)), 1, OK, 100000, OK, OK, None))
row("frame_ranges-n_blocks-wrong", "BAD_ARG", fr(ranges((0, 16, 0)), i=info(n_blocks=3)))
row("frame_ranges-null-out", "BAD_ARG", fr(ranges((0, 16, 0)), out=None))
row("frame_ranges-past-n_total", "BAD_ARG", fr(ranges((99990, 16, 0))))
row("frame_ranges-destination-past-out_cap", "DST_TOO_SMALL", fr(ranges((0, 16, 99990))))
row("frame_ranges-destinations-overlap", "BAD_ARG", fr(ranges((0, 16, 0), (64, 16, 8)), n_ranges=2))
row("frame_range-past-n_total", "BAD_ARG",
    lambda lib: lib.fsehip_frame_decompress_range(info(), 0, OK, 1 << 20, 99990, 16, OK, 100000, OK, None))

# fsehip_bitstack_write(d_vals, d_nbits, count, d_out, out_cap, d_total_bits, stream)
row("dev_bitstack_write-null-out", "BAD_ARG", lambda lib: lib.fsehip_bitstack_write(OK, OK, 4, None, 64, OK, None))
row("dev_bitstack_write-null-total_bits", "BAD_ARG", lambda lib: lib.fsehip_bitstack_write(OK, OK, 4, OK, 64, None, None))
row("dev_bitstack_write-null-vals", "BAD_ARG", lambda lib: lib.fsehip_bitstack_write(None, OK, 4, OK, 64, OK, None))
row("dev_bitstack_write-out-off-by-2", "BAD_ARG", lambda lib: lib.fsehip_bitstack_write(OK, OK, 4, ODD2, 64, OK, None))
# fsehip_bitstack_read(d_in, n_bytes, d_nbits, count, d_vals, d_result, stream)
row("dev_bitstack_read-null-result", "BAD_ARG", lambda lib: lib.fsehip_bitstack_read(OK, 8, OK, 4, OK, None, None))
row("dev_bitstack_read-null-nbits", "BAD_ARG", lambda lib: lib.fsehip_bitstack_read(OK, 8, None, 4, OK, OK, None))
row("dev_bitstack_read-null-in", "BAD_ARG", lambda lib: lib.fsehip_bitstack_read(None, 8, OK, 4, OK, OK, None))
# fsehip_bitstream_read_ops(d_in, n_bytes, total_bits, d_nbits, d_ops, count, d_vals, d_result, stream)
row("dev_bitstream_read_ops-no-bytes", "BAD_ARG", lambda lib: lib.fsehip_bitstream_read_ops(OK, 0, 0, OK, OK, 4, OK, OK, None))
row("dev_bitstream_read_ops-total_bits-mismatch", "BAD_ARG", lambda lib: lib.fsehip_bitstream_read_ops(OK, 8, 65, OK, OK, 4, OK, OK, None))
row("dev_bitstream_read_ops-null-result", "BAD_ARG", lambda lib: lib.fsehip_bitstream_read_ops(OK, 8, 64, OK, OK, 4, OK, None, None))
row("dev_bitstream_read-total_bits-mismatch", "BAD_ARG", lambda lib: lib.fsehip_bitstream_read(OK, 8, 65, OK, 4, OK, OK, None))
row("dev_bitstream_read-null-result", "BAD_ARG", lambda lib: lib.fsehip_bitstream_read(OK, 8, 64, OK, 4, OK, None, None))

# fse_compress2 / fse_compress (src, n, dst, dst_cap, dst_len, payload_bits), fse_compress2_log (+ table_log)
for name, extra in (("fse_compress2", ()), ("fse_compress", ()), ("fse_compress2_log", (9,))):
    def comp(n, dst_len, name=name, extra=extra):
        return lambda lib: getattr(lib, name)(OK, n, *extra, OK, 1 << 20, dst_len, None)
    row(f"{name}-null-dst_len", "BAD_ARG", comp(1000, None))
    row(f"{name}-null-dst_len-before-empty", "BAD_ARG", comp(0, None))
    row(f"{name}-empty", "EMPTY", comp(0, size()))
    row(f"{name}-too-long", "UNSUPPORTED", comp((1 << 28) + 1, size()))

# fse_decompress2 / fse_decompress (src, n, dst, dst_cap, dst_len)
for name in ("fse_decompress2", "fse_decompress"):
    def dec(n, dst_len, name=name):
        return lambda lib: getattr(lib, name)(OK, n, OK, 1000, dst_len)
    row(f"{name}-null-dst_len", "BAD_ARG", dec(100, None))
    row(f"{name}-dst_len-above-dst_cap", "BAD_ARG", dec(100, size(1001)))
    row(f"{name}-dst_len-before-empty", "BAD_ARG", dec(0, size(1001)))
    row(f"{name}-empty", "EMPTY", dec(0, size()))
    row(f"{name}-too-long", "UNSUPPORTED", dec((1 << 30) + 1, size()))

# fse_decompress*_many(srcs, src_lens, n_streams, dst, dst_stride, dst_lens, statuses)
for name in ("fse_decompress2_many", "fse_decompress_many"):
    def dm(srcs=OK, n=4, stride=4096, statuses=OK, name=name):
        return lambda lib: getattr(lib, name)(srcs, OK, n, OK, stride, OK, statuses)
    row(f"{name}-no-streams", "OK", dm(n=0))
    row(f"{name}-no-streams-before-null", "OK", dm(n=0, srcs=None))
    row(f"{name}-null-srcs", "BAD_ARG", dm(srcs=None))
    row(f"{name}-null-statuses", "BAD_ARG", dm(statuses=None))
    row(f"{name}-dst_stride-0", "BAD_ARG", dm(stride=0))
    row(f"{name}-too-many", "UNSUPPORTED", dm(n=(1 << 24) + 1))
    row(f"{name}-dst_stride-2^31", "UNSUPPORTED", dm(stride=1 << 31))
    row(f"{name}-null-before-too-many", "BAD_ARG", dm(srcs=None, n=(1 << 24) + 1))

# fse_compress*_many(srcs, src_lens, n_streams, dst, dst_stride, dst_lens, payload_bits, statuses)
for name in ("fse_compress2_many", "fse_compress_many"):
    def cm(srcs=OK, n=4, stride=4096, statuses=OK, name=name):
        return lambda lib: getattr(lib, name)(srcs, OK, n, OK, stride, OK, None, statuses)
    row(f"{name}-no-streams", "OK", cm(n=0))
    row(f"{name}-no-streams-before-null", "OK", cm(n=0, srcs=None))
    row(f"{name}-null-srcs", "BAD_ARG", cm(srcs=None))
    row(f"{name}-null-statuses", "BAD_ARG", cm(statuses=None))
    row(f"{name}-dst_stride-0", "BAD_ARG", cm(stride=0))
    row(f"{name}-too-many", "UNSUPPORTED", cm(n=(1 << 24) + 1))
    row(f"{name}-null-before-too-many", "BAD_ARG", cm(srcs=None, n=(1 << 24) + 1))

# the building blocks
HIST = _lib.Histogram()
HIST.size, HIST.table_len = 100, 4
HIST257 = _lib.Histogram()
HIST257.size, HIST257.table_len = 100, 257
NORM = _lib.NormHistogram()
NOUT = C.byref(_lib.NormHistogram())
row("histogram_count-null-counts", "BAD_ARG", lambda lib: lib.histogram_count(OK, 100, None, None))
row("histogram_count-n-2^32", "BAD_ARG", lambda lib: lib.histogram_count(OK, 1 << 32, OK, None))
row("histogram_new-null-out", "BAD_ARG", lambda lib: lib.histogram_new(OK, 100, None))
row("histogram_new-n-2^32", "BAD_ARG", lambda lib: lib.histogram_new(OK, 1 << 32, C.byref(_lib.Histogram())))
row("histogram_normalize-null-h", "BAD_ARG", lambda lib: lib.histogram_normalize(None, 9, NOUT))
row("histogram_normalize-table_len-257", "BAD_ARG", lambda lib: lib.histogram_normalize(C.byref(HIST257), 9, NOUT))
row("histogram_normalize-null-out", "BAD_ARG", lambda lib: lib.histogram_normalize(C.byref(HIST), 9, None))
row("histogram_normalize_optimal-null-h", "BAD_ARG", lambda lib: lib.histogram_normalize_optimal(None, NOUT))
row("histogram_normalize_optimal-table_len-257", "BAD_ARG", lambda lib: lib.histogram_normalize_optimal(C.byref(HIST257), NOUT))
row("histogram_normalize_optimal-null-out", "BAD_ARG", lambda lib: lib.histogram_normalize_optimal(C.byref(HIST), None))
row("norm_histogram_new-null-src", "BAD_ARG", lambda lib: lib.norm_histogram_new(None, 3, NOUT))
row("norm_histogram_new-null-out", "BAD_ARG", lambda lib: lib.norm_histogram_new(OK, 3, None))
row("norm_histogram_new-n-2^32", "BAD_ARG", lambda lib: lib.norm_histogram_new(OK, 1 << 32, NOUT))
row("norm_histogram_write-dst_len-above-dst_cap", "BAD_ARG", lambda lib: lib.norm_histogram_write(C.byref(NORM), OK, 10, size(11), None))
row("norm_histogram_write-null-nh", "BAD_ARG", lambda lib: lib.norm_histogram_write(None, OK, 10, size(), None))
row("norm_histogram_write-null-dst_len", "BAD_ARG", lambda lib: lib.norm_histogram_write(C.byref(NORM), OK, 10, None, None))
row("norm_histogram_read-empty", "EMPTY", lambda lib: lib.norm_histogram_read(OK, 0, NOUT, None))
row("norm_histogram_read-null-out", "BAD_ARG", lambda lib: lib.norm_histogram_read(OK, 10, None, None))
row("norm_histogram_read-null-out-before-empty", "BAD_ARG", lambda lib: lib.norm_histogram_read(OK, 0, None, None))
row("norm_histogram_read-null-src", "BAD_ARG", lambda lib: lib.norm_histogram_read(None, 10, NOUT, None))
row("encode_table_new-null-nh", "BAD_ARG", lambda lib: lib.encode_table_new(None, C.cast(OK, C.POINTER(_lib.EncodeTable))))
row("encode_table_new-null-out", "BAD_ARG", lambda lib: lib.encode_table_new(C.byref(NORM), None))
row("decode_table_new-null-nh", "BAD_ARG", lambda lib: lib.decode_table_new(None, C.cast(OK, C.POINTER(_lib.DecodeTable))))
row("decode_table_new-null-out", "BAD_ARG", lambda lib: lib.decode_table_new(C.byref(NORM), None))
row("fse_compress_nh-null-dst_len", "BAD_ARG", lambda lib: lib.fse_compress_nh(OK, 100, OK, 1000, None, None, NOUT))
row("fse_compress_nh-empty", "EMPTY", lambda lib: lib.fse_compress_nh(OK, 0, OK, 1000, size(), None, NOUT))

# the host bit calls
# bitstack_write(vals, nbits, count, dst, dst_cap, dst_len, bits_written)
row("bitstack_write-null-dst_len", "BAD_ARG", lambda lib: lib.bitstack_write(OK, OK, 2, OK, 64, None, None))
row("bitstack_write-dst_len-above-dst_cap", "BAD_ARG", lambda lib: lib.bitstack_write(OK, OK, 2, OK, 64, size(65), None))
row("bitstack_write-null-vals", "BAD_ARG", lambda lib: lib.bitstack_write(None, OK, 2, OK, 64, size(), None))
# bitstack_read(src, n, nbits, count, vals, n_read, finished)
row("bitstack_read-null-nbits", "BAD_ARG", lambda lib: lib.bitstack_read(OK, 8, None, 2, OK, None, None))
row("bitstack_read-null-src", "BAD_ARG", lambda lib: lib.bitstack_read(None, 8, OK, 2, OK, None, None))
# bitstream_read(src, n, total_bits, nbits, count, vals, n_read, bits_left)
row("bitstream_read-null-nbits", "BAD_ARG", lambda lib: lib.bitstream_read(OK, 8, 64, None, 2, OK, None, None))
row("bitstream_read-null-vals", "BAD_ARG", lambda lib: lib.bitstream_read(OK, 8, 64, OK, 2, None, None, None))
# bitstream_read_ops(src, n, total_bits, nbits, ops, count, vals, n_done, bits_left): the ops are read on the host
OPS = (C.c_uint8 * 2)(0, 3)
row("bitstream_read_ops-op-3", "BAD_ARG", lambda lib: lib.bitstream_read_ops(OK, 8, 64, OK, OPS, 2, OK, None, None))
row("bitstream_read_ops-null-nbits", "BAD_ARG", lambda lib: lib.bitstream_read_ops(OK, 8, 64, None, None, 2, OK, None, None))


def test_no_row_reaches_the_device():
    """The rule of the table: a row's status is decided before device_ok()."""
    names = [p.id for p in ROWS]
    assert len(set(names)) == len(names)
    assert all(p.values[1] in _lib.STATUS.values() and p.values[1] not in ("NO_DEVICE", "HIP") for p in ROWS)


@pytest.mark.parametrize("call,want", ROWS)
def test_malformed_call(call, want):
    assert _lib.STATUS[call(_lib.load())] == want
