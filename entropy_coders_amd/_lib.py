"""Loader for the in-tree HIP library libfsehip.so (the product).

There is no CPU fallback: if the library is missing or no HIP device is
usable, calls raise.  Build with ``make -C entropy_coders_amd`` or
``__graft_entry__.build()``.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# FSEHIP_LIB: an alternative in-tree build of the same library for the
# diagnostics in tools/ -- libfsehip_diag.so (`make diag`: the environment
# knobs compiled in) or an A/B variant libfsehip_NAME.so
# (tools/variant_build.sh).  Only a bare libfsehip_*.so name beside this file
# is accepted; the product is libfsehip.so, which reads no environment.
_LIB_NAME = os.environ.get("FSEHIP_LIB", "libfsehip.so")
if _LIB_NAME != "libfsehip.so" and not (
        _LIB_NAME.startswith("libfsehip_") and _LIB_NAME.endswith(".so") and os.sep not in _LIB_NAME):
    raise RuntimeError(f"FSEHIP_LIB={_LIB_NAME!r}: expected libfsehip_NAME.so (an in-tree variant build)")
LIB_PATH = os.path.join(HERE, _LIB_NAME)

# every symbol include/fsehip.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "fse_compress2", "fse_compress2_log", "fse_decompress2", "histogram_count",
    "fsehip_slot_bytes", "fsehip_sidecar_per_block", "fsehip_compress_blocks",
    "fsehip_decompress_blocks", "fsehip_build_sidecar", "fsehip_decompress_streams", "fsehip_histogram_blocks",
    "fsehip_generate", "fsehip_device_count", "fsehip_version",
    "fsehip_pack_blocks", "fsehip_unpack_blocks",
    "fsehip_dtable_bytes", "fsehip_build_dtables", "fsehip_decompress_blocks_dt",
    "fse_compress", "fse_decompress", "fsehip_sidecar_per_block_ns", "fse_decompress2_many", "fse_decompress_many",
    "fsehip_copy_blocks", "fsehip_release_workspace", "fsehip_rank_fallbacks",
    "histogram_new", "histogram_normalize", "histogram_normalize_optimal", "norm_histogram_new",
    "norm_histogram_write", "norm_histogram_read", "encode_table_new", "decode_table_new", "fse_compress_nh",
    "bitstack_write", "bitstack_read", "bitstream_read", "bitstream_read_ops",
    "fsehip_bitstack_write", "fsehip_bitstack_read", "fsehip_bitstream_read", "fsehip_bitstream_read_ops",
    "bitstack_reader_new", "bitstack_reader_reload", "bitstack_reader_peek", "bitstack_reader_read_no_reload",
    "bitstack_reader_advance_no_reload", "bitstack_reader_read", "bitstack_reader_available", "bitstack_reader_finish",
    "bitstream_reader_new", "bitstream_reader_read", "bitstream_reader_advance_by", "bitstream_reader_peek",
    "bitstream_reader_available", "bitstream_reader_finish", "bitstream_reader_finish_byte",
    "bitstack_writer_new", "bitstack_writer_flush", "bitstack_writer_write_bits_raw",
    "bitstack_writer_write_bits_raw_unmasked", "bitstack_writer_write_bits", "bitstack_writer_write_bits_unmasked",
    "bitstack_writer_finish",
    "fse_compress2_many", "fse_compress_many", "fsehip_compress_streams", "fsehip_stream_out_bytes",
    "fsehip_frame_bound", "fsehip_frame_read_header", "fsehip_frame_write_header",
    "fsehip_frame_compress", "fsehip_frame_decompress",
    "fsehip_frame_decompress_ranges", "fsehip_frame_decompress_range",
    "norm_histogram_try_from", "fsehip_shared_table_bytes", "fsehip_shared_table_build", "fsehip_shared_out_bytes",
    "fsehip_compress_shared", "fsehip_decompress_shared",
    "fsehip_planes_bound", "fsehip_planes_scratch_bytes", "fsehip_planes_read_header", "fsehip_planes_write_header",
    "fsehip_planes_split", "fsehip_planes_merge", "fsehip_planes_compress", "fsehip_planes_decompress",
    "fsehip_planes_ranges_scratch_bytes", "fsehip_planes_decompress_ranges",
    "fsehip_delta_bound", "fsehip_delta_scratch_bytes", "fsehip_delta_read_header", "fsehip_delta_write_header",
    "fsehip_delta_encode", "fsehip_delta_decode", "fsehip_delta_compress", "fsehip_delta_decompress",
    "fsehip_delta_ranges_scratch_bytes", "fsehip_delta_decompress_ranges",
    "fsehip_diff_bound", "fsehip_diff_scratch_bytes", "fsehip_diff_read_header", "fsehip_diff_write_header",
    "fsehip_diff_encode", "fsehip_diff_decode", "fsehip_diff_compress", "fsehip_diff_decompress",
    "fsehip_diff_ranges_scratch_bytes", "fsehip_diff_decompress_ranges",
    "fsehip_crc32", "fsehip_crc32_combine", "fsehip_check_bytes", "fsehip_check_read_header",
    "fsehip_check_write_header", "fsehip_sealed_read_header", "fsehip_check_build", "fsehip_check_verify",
    "fsehip_check_ranges_verified_bytes", "fsehip_check_verify_ranges",
    "fsehip_log2q8", "fsehip_estimate_choose", "fsehip_estimate_block_host", "fsehip_container_kind",
    "fsehip_estimate_image_bytes", "fsehip_image_histogram", "fsehip_estimate_blocks",
    "fsehip_estimate_scratch_bytes", "fsehip_estimate",
    "fsehip_diff_image_histogram", "fsehip_estimate_base_scratch_bytes", "fsehip_estimate_base",
    "fsehip_estimate_choose_base",
    "fsehip_pack_image_bytes", "fsehip_pack_bound", "fsehip_pack_scratch_bytes", "fsehip_pack_members_scratch_bytes",
    "fsehip_pack_plane_offset", "fsehip_pack_read_header", "fsehip_pack_read_members", "fsehip_pack_write_header",
    "fsehip_pack_split", "fsehip_pack_merge", "fsehip_pack_compress", "fsehip_pack_decompress",
    "fsehip_pack_decompress_members",
    "fsehip_vpack_image_bytes", "fsehip_vpack_bound", "fsehip_vpack_scratch_bytes",
    "fsehip_vpack_members_scratch_bytes", "fsehip_vpack_plane_offset", "fsehip_vpack_read_header",
    "fsehip_vpack_read_members", "fsehip_vpack_write_header", "fsehip_vpack_split", "fsehip_vpack_merge",
    "fsehip_vpack_compress", "fsehip_vpack_decompress", "fsehip_vpack_decompress_members",
    "fsehip_mcheck_bytes", "fsehip_mcheck_read_header", "fsehip_mcheck_write_header", "fsehip_spack_read_header",
    "fsehip_mcheck_scratch_bytes", "fsehip_spack_bound", "fsehip_spack_scratch_bytes",
    "fsehip_spack_members_scratch_bytes", "fsehip_mcheck_build", "fsehip_mcheck_verify", "fsehip_spack_compress",
    "fsehip_spack_decompress", "fsehip_spack_decompress_members",
)

STATUS = {
    0: "OK", -1: "EMPTY", -2: "TOO_SHORT", -3: "ALL_ZERO_SYMBOL0", -4: "SINGLE_SYMBOL",
    -5: "BAD_HEADER", -6: "NO_MARKER", -7: "DST_TOO_SMALL", -8: "TABLELOG_RANGE",
    -9: "CURSED", -10: "BAD_TABLE", -11: "BAD_ARG", -12: "HIP", -13: "LENGTH_MISMATCH",
    -14: "UNSUPPORTED", -15: "NO_DEVICE", -16: "BAD_SIDECAR", -17: "ENCODER_INIT",
    -18: "EOF", -19: "BAD_FRAME", -20: "SYMBOL_NOT_IN_TABLE", -21: "CHECKSUM",
}


class FseError(Exception):
    """A negative status from the C ABI (a reference panic/None/Err)."""

    def __init__(self, rc: int, what: str = ""):
        self.rc = rc
        self.code = STATUS.get(rc, str(rc))
        super().__init__(f"{what}: status {rc} ({self.code})" if what else f"status {rc} ({self.code})")


class Params(C.Structure):
    _fields_ = [("block_size", C.c_uint32), ("table_log", C.c_uint32),
                ("ckpt_interval", C.c_uint32), ("max_table_log", C.c_uint32),
                ("nstates", C.c_uint32)]


class StreamDesc(C.Structure):
    """fsehip_stream_desc: one stream of fsehip_compress_streams."""
    _fields_ = [("src_off", C.c_uint64), ("out_off", C.c_uint64), ("src_len", C.c_uint32), ("out_cap", C.c_uint32)]


class FrameInfo(C.Structure):
    """fsehip_frame_info: a frame's header fields, records_off = 32 + 4 * n_blocks."""
    _fields_ = [("version", C.c_uint32), ("nstates", C.c_uint32), ("max_table_log", C.c_uint32),
                ("flags", C.c_uint32), ("block_size", C.c_uint32), ("ckpt_interval", C.c_uint32),
                ("n_blocks", C.c_uint32), ("reserved", C.c_uint32), ("n_total", C.c_uint64),
                ("records_off", C.c_uint64)]


class FrameRange(C.Structure):
    """fsehip_frame_range: raw bytes [src_off, src_off + len) go to d_out + dst_off."""
    _fields_ = [("src_off", C.c_uint64), ("len", C.c_uint64), ("dst_off", C.c_uint64)]


class FrameParams(C.Structure):
    """fsehip_frame_params: fsehip_params + chunk_blocks (0 = 4096)."""
    _fields_ = [("block_size", C.c_uint32), ("table_log", C.c_uint32), ("ckpt_interval", C.c_uint32),
                ("max_table_log", C.c_uint32), ("nstates", C.c_uint32), ("chunk_blocks", C.c_uint32)]


class PlanesInfo(C.Structure):
    """fsehip_planes_info: a plane, delta or diff frame's header fields, stride = roundup(n_elems, 16)."""
    _fields_ = [("version", C.c_uint32), ("elem_bytes", C.c_uint32), ("reserved", C.c_uint32), ("pad_", C.c_uint32),
                ("n_elems", C.c_uint64), ("stride", C.c_uint64)]


class PlanesRange(C.Structure):
    """fsehip_planes_range: elements [elem_off, elem_off + n_elems) go to element dst_elem_off of d_out."""
    _fields_ = [("elem_off", C.c_uint64), ("n_elems", C.c_uint64), ("dst_elem_off", C.c_uint64)]


DELTA_RESTART = 4096  # FSEHIP_DELTA_RESTART: elements between the delta frame's restarts


DeltaInfo = PlanesInfo  # fsehip_delta_info is a typedef of fsehip_planes_info
DiffInfo = PlanesInfo   # and so is fsehip_diff_info


CHECK_CRC32 = 1  # FSEHIP_CHECK_CRC32: the check record's algorithm
SEALED_KINDS = ("frame", "planes", "delta", "diff")  # FSEHIP_SEALED_FRAME / _PLANES / _DELTA / _DIFF


class CheckInfo(C.Structure):
    """fsehip_check_info: a check record's header fields; the table follows at byte 32."""
    _fields_ = [("version", C.c_uint32), ("algorithm", C.c_uint32), ("check_log", C.c_uint32), ("reserved", C.c_uint32),
                ("n_content", C.c_uint64), ("n_cb", C.c_uint32), ("content_crc", C.c_uint32),
                ("header_crc", C.c_uint32), ("pad_", C.c_uint32)]


KINDS = ("frame", "planes", "delta")  # FSEHIP_KIND_FRAME / _PLANES / _DELTA
KIND_SEALED = 3                        # FSEHIP_KIND_SEALED: fsehip_container_kind of an "FSEK" buffer
KIND_DIFF = 4                          # FSEHIP_KIND_DIFF: of an "FSEB" buffer; fsehip_estimate_base's fifth entry
KIND_PACK = 5                          # FSEHIP_KIND_PACK: of an "FSEM" buffer
KIND_VPACK = 6                         # FSEHIP_KIND_VPACK: of an "FSEV" buffer
KIND_SPACK = 7                         # FSEHIP_KIND_SPACK: of an "FSES" buffer
MCHECK_BASES = 1                       # FSEHIP_MCHECK_BASES: the member check record's flag bit 0
PACK_MAX_MEMBERS = 1 << 20             # FSEHIP_PACK_MAX_MEMBERS
EST_NONE = (1 << 64) - 1               # FSEHIP_EST_NONE
EST_RAW, EST_RLE, EST_FSE = 0, 1, 2    # FSEHIP_EST_*: the frame directory's block types


class PackMember(C.Structure):
    """fsehip_pack_member: one tensor of a pack frame; kind is 1 (planes) or 2 (delta), in a versioned pack also 4 (diff)."""
    _fields_ = [("d_ptr", C.c_void_p), ("n_elems", C.c_uint64), ("elem_bytes", C.c_uint32), ("kind", C.c_uint32)]


class PackInfo(C.Structure):
    """fsehip_pack_info: a pack frame's header fields; the member table follows at byte 32."""
    _fields_ = [("version", C.c_uint32), ("n_members", C.c_uint32), ("image_bytes", C.c_uint64),
                ("content_bytes", C.c_uint64)]


class McheckInfo(C.Structure):
    """fsehip_mcheck_info: a member check record's header fields; the table (8 bytes per member) follows at byte 32."""
    _fields_ = [("version", C.c_uint32), ("algorithm", C.c_uint32), ("flags", C.c_uint32), ("n_members", C.c_uint32),
                ("content_bytes", C.c_uint64), ("header_crc", C.c_uint32), ("reserved", C.c_uint32)]


class BlockEstimate(C.Structure):
    """fsehip_block_estimate: one block's estimated type, record bytes, payload bits and table log."""
    _fields_ = [("type", C.c_uint32), ("rec", C.c_uint32), ("bits", C.c_uint32), ("table_log", C.c_uint32)]


class Histogram(C.Structure):
    """fse_histogram = Histogram (histogram.rs:9-14)."""
    _fields_ = [("counts", C.c_uint32 * 256), ("size", C.c_uint32), ("table_len", C.c_uint32)]


class NormHistogram(C.Structure):
    """fse_norm_histogram = NormHistogram (histogram.rs:289-294)."""
    _fields_ = [("norm", C.c_int32 * 256), ("log2", C.c_uint32), ("table_len", C.c_uint32)]


class SymbolTransform(C.Structure):
    _fields_ = [("bits", C.c_uint32), ("find_state", C.c_int32)]


class EncodeTable(C.Structure):
    """fse_encode_table = EncodeTable (fse.rs:72-84)."""
    _fields_ = [("table_log", C.c_uint32), ("table", C.c_uint16 * 32768), ("symbols", C.c_uint8 * 32768),
                ("symbol_tt", SymbolTransform * 256)]


class DecodeTransform(C.Structure):
    _fields_ = [("new_state", C.c_uint16), ("symbol", C.c_uint8), ("num_bits", C.c_uint8)]


class DecodeTable(C.Structure):
    """fse_decode_table = DecodeTable (fse.rs:253-265)."""
    _fields_ = [("table_log", C.c_uint32), ("fast_mode", C.c_uint32), ("table", DecodeTransform * 32768)]


class BitStackReaderState(C.Structure):
    """fse_bitstack_reader = BitStackReader (stack_reader.rs:5-11)."""
    _fields_ = [("base", C.c_void_p), ("ptr", C.c_void_p), ("buffer", C.c_uint64), ("bits", C.c_uint64),
                ("finished", C.c_int32), ("reserved", C.c_int32)]


class BitStreamReaderState(C.Structure):
    """fse_bitstream_reader = BitStreamReader (stream_reader.rs:5-11)."""
    _fields_ = [("src", C.c_void_p), ("n", C.c_uint64), ("total_bits", C.c_uint64), ("bits_read", C.c_uint64)]


class BitStackWriterState(C.Structure):
    """fse_bitstack_writer = BitStackWriter (writer.rs:5-12)."""
    _fields_ = [("dst", C.c_void_p), ("cap", C.c_uint64), ("len", C.c_uint64), ("initial_len", C.c_uint64),
                ("storage", C.c_uint64), ("bits", C.c_uint32), ("status", C.c_int32)]


_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build the HIP extension first "
                           "(make -C entropy_coders_amd); there is no CPU fallback")
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so.7 /
    # libhsa-runtime64.so.1 and loads them by path; loaded first, the
    # library's DT_NEEDED entries (same sonames) resolve to torch's copies.
    # Loaded the other way round, /opt/rocm's runtime comes in first and torch
    # then finds no GPU ("No HIP GPUs are available", seen when a test called
    # the library before touching torch).  So torch, when installed, goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    P, sz, u32, u64, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int32
    lib.fse_compress2.argtypes = [P, sz, P, sz, C.POINTER(sz), C.POINTER(u64)]
    lib.fse_compress2_log.argtypes = [P, sz, u32, P, sz, C.POINTER(sz), C.POINTER(u64)]
    lib.fse_decompress2.argtypes = [P, sz, P, sz, C.POINTER(sz)]
    lib.fse_compress.argtypes = [P, sz, P, sz, C.POINTER(sz), C.POINTER(u64)]
    lib.fse_decompress.argtypes = [P, sz, P, sz, C.POINTER(sz)]
    lib.fse_decompress2_many.argtypes = [P, P, sz, P, sz, P, P]
    lib.fse_decompress_many.argtypes = [P, P, sz, P, sz, P, P]
    lib.fse_compress2_many.argtypes = [P, P, sz, P, sz, P, P, P]
    lib.fse_compress_many.argtypes = [P, P, sz, P, sz, P, P, P]
    lib.fsehip_compress_streams.argtypes = [u32, u32, u32, P, P, u32, P, P, P, P, P]
    lib.fsehip_stream_out_bytes.argtypes = [u32, u32]
    lib.fsehip_stream_out_bytes.restype = u64
    lib.histogram_count.argtypes = [P, sz, P, C.POINTER(u32)]
    lib.fsehip_slot_bytes.argtypes = [u32, u32]
    lib.fsehip_slot_bytes.restype = u64
    lib.fsehip_sidecar_per_block.argtypes = [u32, u32]
    lib.fsehip_sidecar_per_block.restype = u32
    lib.fsehip_sidecar_per_block_ns.argtypes = [u32, u32, u32]
    lib.fsehip_sidecar_per_block_ns.restype = u32
    lib.fsehip_compress_blocks.argtypes = [C.POINTER(Params), P, u64, P, u64, P, P, P, P, P]
    lib.fsehip_decompress_blocks.argtypes = [C.POINTER(Params), P, u64, P, P, P, u64, P, P]
    lib.fsehip_build_sidecar.argtypes = [C.POINTER(Params), P, u64, P, P, u64, P, P, P]
    lib.fsehip_decompress_streams.argtypes = [C.c_uint32, C.c_uint32, P, u64, P, C.c_uint32, P, C.c_uint32, P, P, P]
    lib.fsehip_dtable_bytes.argtypes = [u32]
    lib.fsehip_dtable_bytes.restype = u64
    lib.fsehip_build_dtables.argtypes = [C.POINTER(Params), P, u64, P, u32, P, P, P]
    lib.fsehip_decompress_blocks_dt.argtypes = [C.POINTER(Params), P, u64, P, P, P, P, P, u64, P, P]
    lib.fsehip_histogram_blocks.argtypes = [P, u64, u32, P, P, P]
    lib.fsehip_generate.argtypes = [C.c_int, C.c_double, u64, u32, P, u64, P]
    lib.fsehip_pack_blocks.argtypes = [P, u64, P, P, u32, P, P]
    lib.fsehip_unpack_blocks.argtypes = [P, P, P, u32, P, u64, P]
    lib.fsehip_copy_blocks.argtypes = [P, P, P, u32, P, P, P]
    lib.fsehip_release_workspace.argtypes = [C.c_int, P]
    lib.fsehip_frame_bound.argtypes = [u64, u32]
    lib.fsehip_frame_bound.restype = u64
    lib.fsehip_frame_read_header.argtypes = [P, sz, C.POINTER(FrameInfo)]
    lib.fsehip_frame_write_header.argtypes = [C.POINTER(FrameInfo), P]
    lib.fsehip_frame_compress.argtypes = [C.POINTER(FrameParams), P, u64, P, u64, P, P, P]
    lib.fsehip_frame_decompress.argtypes = [C.POINTER(FrameInfo), u32, P, u64, P, u64, P, P, P]
    lib.fsehip_frame_decompress_ranges.argtypes = [C.POINTER(FrameInfo), u32, P, u64, C.POINTER(FrameRange), u32, P, u64,
                                                   P, P, P]
    lib.fsehip_frame_decompress_range.argtypes = [C.POINTER(FrameInfo), u32, P, u64, u64, u64, P, u64, P, P]
    # the plane and the delta frame: the same ten prototypes under two
    # prefixes, but for the names of the two bare transforms
    PI, FI, PR = C.POINTER(PlanesInfo), C.POINTER(FrameInfo), C.POINTER(PlanesRange)
    for prefix, split, merge in (("fsehip_planes_", "split", "merge"), ("fsehip_delta_", "encode", "decode")):
        fn = lambda name, prefix=prefix: getattr(lib, prefix + name)  # noqa: E731
        fn("bound").argtypes = [u64, u32, u32]
        fn("bound").restype = u64
        fn("scratch_bytes").argtypes = [u64, u32]
        fn("scratch_bytes").restype = u64
        fn("read_header").argtypes = [P, sz, PI, FI]
        fn("write_header").argtypes = [PI, P]
        fn(split).argtypes = [u32, P, u64, P, P]
        fn(merge).argtypes = [u32, P, u64, P, P]
        fn("compress").argtypes = [C.POINTER(FrameParams), u32, P, u64, P, u64, P, u64, P, P, P]
        fn("decompress").argtypes = [PI, FI, u32, P, u64, P, u64, P, u64, P, P, P]
        fn("ranges_scratch_bytes").argtypes = [u32, PR, u32]
        fn("ranges_scratch_bytes").restype = u64
        fn("decompress_ranges").argtypes = [PI, FI, u32, P, u64, PR, u32, P, u64, P, u64, P, P, P]
    # the diff frame: the same ten, with the base after the source or destination pointer
    lib.fsehip_diff_bound.argtypes = [u64, u32, u32]
    lib.fsehip_diff_bound.restype = u64
    lib.fsehip_diff_scratch_bytes.argtypes = [u64, u32]
    lib.fsehip_diff_scratch_bytes.restype = u64
    lib.fsehip_diff_read_header.argtypes = [P, sz, PI, FI]
    lib.fsehip_diff_write_header.argtypes = [PI, P]
    lib.fsehip_diff_encode.argtypes = [u32, P, P, u64, P, P]
    lib.fsehip_diff_decode.argtypes = [u32, P, u64, P, P, P]
    lib.fsehip_diff_compress.argtypes = [C.POINTER(FrameParams), u32, P, P, u64, P, u64, P, u64, P, P, P]
    lib.fsehip_diff_decompress.argtypes = [PI, FI, u32, P, u64, P, u64, P, P, u64, P, P, P]
    lib.fsehip_diff_ranges_scratch_bytes.argtypes = [u32, PR, u32]
    lib.fsehip_diff_ranges_scratch_bytes.restype = u64
    lib.fsehip_diff_decompress_ranges.argtypes = [PI, FI, u32, P, u64, PR, u32, P, u64, P, P, u64, P, P, P]
    CI = C.POINTER(CheckInfo)
    lib.fsehip_crc32.argtypes = [u32, P, sz]
    lib.fsehip_crc32.restype = u32
    lib.fsehip_crc32_combine.argtypes = [u32, u32, u64]
    lib.fsehip_crc32_combine.restype = u32
    lib.fsehip_check_bytes.argtypes = [u64, u32]
    lib.fsehip_check_bytes.restype = u64
    lib.fsehip_check_read_header.argtypes = [P, sz, CI]
    lib.fsehip_check_write_header.argtypes = [CI, P]
    lib.fsehip_sealed_read_header.argtypes = [P, sz, CI, C.POINTER(u32), C.POINTER(u64)]
    lib.fsehip_check_build.argtypes = [u32, P, u64, P, P]
    lib.fsehip_check_verify.argtypes = [CI, P, P, u64, P, P, P]
    lib.fsehip_check_ranges_verified_bytes.argtypes = [CI, C.POINTER(FrameRange), u32, C.POINTER(u64)]
    lib.fsehip_check_verify_ranges.argtypes = [CI, P, C.POINTER(FrameRange), u32, P, u64, P, P, P]
    lib.fsehip_log2q8.argtypes = [u32]
    lib.fsehip_log2q8.restype = u32
    lib.fsehip_estimate_choose.argtypes = [C.POINTER(u64 * 3)]
    lib.fsehip_estimate_block_host.argtypes = [P, u32, P, u32, u32, C.POINTER(FrameParams), C.POINTER(BlockEstimate)]
    lib.fsehip_container_kind.argtypes = [P, sz]
    lib.fsehip_estimate_image_bytes.argtypes = [u32, u64, u32]
    lib.fsehip_estimate_image_bytes.restype = u64
    lib.fsehip_image_histogram.argtypes = [u32, u32, P, u64, u32, P, P]
    lib.fsehip_estimate_blocks.argtypes = [C.POINTER(FrameParams), P, u64, P, P, P, P, P, P]
    lib.fsehip_estimate_scratch_bytes.argtypes = [u64, u32, u32, u32]
    lib.fsehip_estimate_scratch_bytes.restype = u64
    lib.fsehip_estimate.argtypes = [C.POINTER(FrameParams), u32, u32, P, u64, P, u64, P, P]
    lib.fsehip_diff_image_histogram.argtypes = [u32, P, P, u64, u32, P, P]
    lib.fsehip_estimate_base_scratch_bytes.argtypes = [u64, u32, u32, u32]
    lib.fsehip_estimate_base_scratch_bytes.restype = u64
    lib.fsehip_estimate_base.argtypes = [C.POINTER(FrameParams), u32, u32, P, P, u64, P, u64, P, P]
    lib.fsehip_estimate_choose_base.argtypes = [C.POINTER(u64 * 5)]
    PM, PKI = C.POINTER(PackMember), C.POINTER(PackInfo)
    for name in ("image_bytes", "bound", "scratch_bytes", "members_scratch_bytes", "plane_offset"):
        getattr(lib, "fsehip_pack_" + name).restype = u64
    lib.fsehip_pack_image_bytes.argtypes = [PM, u32]
    lib.fsehip_pack_bound.argtypes = [PM, u32, u32]
    lib.fsehip_pack_scratch_bytes.argtypes = [PM, u32]
    lib.fsehip_pack_members_scratch_bytes.argtypes = [PM, u32, C.POINTER(u32), u32]
    lib.fsehip_pack_plane_offset.argtypes = [PM, u32, u32, u32]
    lib.fsehip_pack_read_header.argtypes = [P, sz, PKI]
    lib.fsehip_pack_read_members.argtypes = [P, sz, PM, u32, PKI, FI]
    lib.fsehip_pack_write_header.argtypes = [PM, u32, P]
    lib.fsehip_pack_split.argtypes = [PM, u32, P, P, u64, P]
    lib.fsehip_pack_merge.argtypes = [PM, u32, P, P, u64, P]
    lib.fsehip_pack_compress.argtypes = [C.POINTER(FrameParams), PM, u32, P, u64, P, u64, P, P, P]
    lib.fsehip_pack_decompress.argtypes = [PKI, PM, FI, u32, P, u64, P, u64, P, P, P]
    lib.fsehip_pack_decompress_members.argtypes = [PKI, PM, FI, u32, P, u64, C.POINTER(u32), u32, P, u64, P, P, P]
    # the versioned pack: the same calls, the device ones with the host array of base pointers behind the members
    BP = C.POINTER(C.c_void_p)
    for name in ("image_bytes", "bound", "scratch_bytes", "members_scratch_bytes", "plane_offset"):
        getattr(lib, "fsehip_vpack_" + name).restype = u64
    lib.fsehip_vpack_image_bytes.argtypes = [PM, u32]
    lib.fsehip_vpack_bound.argtypes = [PM, u32, u32]
    lib.fsehip_vpack_scratch_bytes.argtypes = [PM, u32]
    lib.fsehip_vpack_members_scratch_bytes.argtypes = [PM, u32, C.POINTER(u32), u32]
    lib.fsehip_vpack_plane_offset.argtypes = [PM, u32, u32, u32]
    lib.fsehip_vpack_read_header.argtypes = [P, sz, PKI]
    lib.fsehip_vpack_read_members.argtypes = [P, sz, PM, u32, PKI, FI]
    lib.fsehip_vpack_write_header.argtypes = [PM, u32, P]
    lib.fsehip_vpack_split.argtypes = [PM, u32, BP, P, P, u64, P]
    lib.fsehip_vpack_merge.argtypes = [PM, u32, BP, P, P, u64, P]
    lib.fsehip_vpack_compress.argtypes = [C.POINTER(FrameParams), PM, u32, BP, P, u64, P, u64, P, P, P]
    lib.fsehip_vpack_decompress.argtypes = [PKI, PM, BP, FI, u32, P, u64, P, u64, P, P, P]
    lib.fsehip_vpack_decompress_members.argtypes = [PKI, PM, BP, FI, u32, P, u64, C.POINTER(u32), u32, P, u64, P, P, P]
    # the member check record and the sealed pack
    MI, pu32_, pu64_ = C.POINTER(McheckInfo), C.POINTER(u32), C.POINTER(u64)
    for name in ("fsehip_mcheck_bytes", "fsehip_mcheck_scratch_bytes", "fsehip_spack_bound",
                 "fsehip_spack_scratch_bytes", "fsehip_spack_members_scratch_bytes"):
        getattr(lib, name).restype = u64
    lib.fsehip_mcheck_bytes.argtypes = [u32]
    lib.fsehip_mcheck_read_header.argtypes = [P, sz, MI]
    lib.fsehip_mcheck_write_header.argtypes = [MI, P]
    lib.fsehip_spack_read_header.argtypes = [P, sz, MI, pu32_, pu64_]
    lib.fsehip_mcheck_scratch_bytes.argtypes = [PM, u32, pu32_, u32, u32]
    lib.fsehip_spack_bound.argtypes = [PM, u32, u32, u32]
    lib.fsehip_spack_scratch_bytes.argtypes = [PM, u32, u32]
    lib.fsehip_spack_members_scratch_bytes.argtypes = [PM, u32, u32, pu32_, u32]
    lib.fsehip_mcheck_build.argtypes = [PM, BP, u32, P, P, u64, P]
    lib.fsehip_mcheck_verify.argtypes = [MI, P, PM, pu32_, u32, u32, BP, P, u64, P, P, P]
    lib.fsehip_spack_compress.argtypes = [C.POINTER(FrameParams), PM, u32, BP, u32, P, u64, P, u64, P, P, P]
    lib.fsehip_spack_decompress.argtypes = [MI, PKI, u32, PM, BP, FI, u32, P, u64, P, u64, P, P, P, P, P, P]
    lib.fsehip_spack_decompress_members.argtypes = [MI, PKI, u32, PM, BP, FI, u32, P, u64, pu32_, u32, P, u64, P, P,
                                                    P, P, P, P]
    lib.fsehip_rank_fallbacks.argtypes = [C.c_int, C.POINTER(u32 * 3), C.c_int]
    lib.norm_histogram_try_from.argtypes = [P, C.POINTER(NormHistogram)]
    lib.fsehip_shared_table_bytes.argtypes = []
    lib.fsehip_shared_table_bytes.restype = u64
    lib.fsehip_shared_table_build.argtypes = [P, P, P, P]
    lib.fsehip_shared_out_bytes.argtypes = [u32, u32]
    lib.fsehip_shared_out_bytes.restype = u64
    lib.fsehip_compress_shared.argtypes = [u32, P, P, P, u32, P, P, P, P, P]
    lib.fsehip_decompress_shared.argtypes = [u32, P, P, P, u32, P, P, P, P, P]
    H, NH = C.POINTER(Histogram), C.POINTER(NormHistogram)
    lib.histogram_new.argtypes = [P, sz, H]
    lib.histogram_normalize.argtypes = [H, u32, NH]
    lib.histogram_normalize_optimal.argtypes = [H, NH]
    lib.norm_histogram_new.argtypes = [P, sz, NH]
    lib.norm_histogram_write.argtypes = [NH, P, sz, C.POINTER(sz), C.POINTER(u64)]
    lib.norm_histogram_read.argtypes = [P, sz, NH, C.POINTER(sz)]
    lib.encode_table_new.argtypes = [NH, C.POINTER(EncodeTable)]
    lib.decode_table_new.argtypes = [NH, C.POINTER(DecodeTable)]
    lib.fse_compress_nh.argtypes = [P, sz, P, sz, C.POINTER(sz), C.POINTER(u64), NH]
    lib.bitstack_write.argtypes = [P, P, sz, P, sz, C.POINTER(sz), C.POINTER(u64)]
    lib.bitstack_read.argtypes = [P, sz, P, sz, P, C.POINTER(sz), C.POINTER(C.c_int)]
    lib.bitstream_read.argtypes = [P, sz, u64, P, sz, P, C.POINTER(sz), C.POINTER(u64)]
    lib.bitstream_read_ops.argtypes = [P, sz, u64, P, P, sz, P, C.POINTER(sz), C.POINTER(u64)]
    lib.fsehip_bitstack_write.argtypes = [P, P, u64, P, u64, P, P]
    lib.fsehip_bitstack_read.argtypes = [P, u64, P, u64, P, P, P]
    lib.fsehip_bitstream_read.argtypes = [P, u64, u64, P, u64, P, P, P]
    lib.fsehip_bitstream_read_ops.argtypes = [P, u64, u64, P, P, u64, P, P, P]
    SR, TR, SW = C.POINTER(BitStackReaderState), C.POINTER(BitStreamReaderState), C.POINTER(BitStackWriterState)
    pu32 = C.POINTER(u32)
    lib.bitstack_reader_new.argtypes = [SR, P, sz]
    lib.bitstack_reader_reload.argtypes = [SR]
    for f in ("peek", "read_no_reload", "read"):
        getattr(lib, "bitstack_reader_" + f).argtypes = [SR, u32, pu32]
    lib.bitstack_reader_advance_no_reload.argtypes = [SR, u32]
    lib.bitstack_reader_available.argtypes = [SR]
    lib.bitstack_reader_available.restype = u64
    lib.bitstack_reader_finish.argtypes = [SR]
    lib.bitstream_reader_new.argtypes = [TR, P, sz, u64]
    lib.bitstream_reader_read.argtypes = [TR, u32, pu32]
    lib.bitstream_reader_peek.argtypes = [TR, u32, pu32]
    lib.bitstream_reader_advance_by.argtypes = [TR, u32]
    lib.bitstream_reader_available.argtypes = [TR]
    lib.bitstream_reader_available.restype = u64
    lib.bitstream_reader_finish.argtypes = [TR, C.POINTER(sz), C.POINTER(u64), pu32]
    lib.bitstream_reader_finish_byte.argtypes = [TR]
    lib.bitstream_reader_finish_byte.restype = sz
    lib.bitstack_writer_new.argtypes = [SW, P, sz, sz]
    lib.bitstack_writer_flush.argtypes = [SW]
    for f in ("write_bits_raw", "write_bits_raw_unmasked", "write_bits", "write_bits_unmasked"):
        getattr(lib, "bitstack_writer_" + f).argtypes = [SW, u32, u32]
    lib.bitstack_writer_finish.argtypes = [SW, C.POINTER(sz), C.POINTER(u64)]
    lib.fsehip_device_count.argtypes = []
    lib.fsehip_version.restype = C.c_char_p
    for name in EXPORTS:
        if getattr(lib, name, None) is None:
            raise RuntimeError(f"libfsehip.so lacks {name}")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise FseError(rc, what)
