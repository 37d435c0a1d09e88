"""The frame format (include/fsehip.h section 2b) restated in numpy over the
CPU oracle: a helper for the frame tests, not a test.

  build_frame   raw bytes -> frame, from O.compress2 / O.compress per block
                plus the encoder rule
  split_frame   frame -> (info dict, directory, records)
  decode_frame  frame -> raw bytes, FSE blocks through the oracle's decoders
  corpus        the inputs the frame tests share

Nothing here calls the library under test.
"""
import struct

import numpy as np

from oracle import oracle as O

MAGIC = b"FSEF"
RAW, RLE, FSE = 0, 1, 2
BAD_FRAME = -19


class FrameError(Exception):
    pass


def n_blocks_of(n_total, block_size):
    return (n_total + block_size - 1) // block_size


def raw_len(n_total, block_size, b):
    return min(block_size, n_total - b * block_size)


def spb_of(n, ckpt, nstates):
    """fsehip_sidecar_per_block_ns."""
    if ckpt == 0:
        return 0
    return n // ckpt + 2 if nstates == 1 else n // 2 // ckpt + 2


def kernel_class(table_log):
    """The header's max_table_log: the kernel class BlockCodec encodes under."""
    return max(11, min(table_log, 15)) if table_log else 11


def slot_bytes(block_size, max_table_log):
    """fsehip_slot_bytes."""
    payload = (block_size * max_table_log + 2 * max_table_log + 1 + 7) // 8
    return (512 + payload + 16 + 255) // 256 * 256


def header(nstates, max_table_log, block_size, ckpt, n_total, n_blocks=None, version=1, flags=None, reserved=0,
           magic=MAGIC):
    if n_blocks is None:
        n_blocks = n_blocks_of(n_total, block_size)
    if flags is None:
        flags = 1 if ckpt else 0
    return magic + struct.pack("<BBBBIIQII", version, nstates, max_table_log, flags, block_size, ckpt, n_total,
                               n_blocks, reserved)


def bound(n_total, block_size):
    return 32 + 4 * n_blocks_of(n_total, block_size) + n_total


def encode_block(s, nstates, table_log):
    """(status name, compressed bytes) of one block on the oracle."""
    try:
        if nstates == 1:
            return "OK", O.compress(s, None if table_log == 0 else table_log)[0]
        return "OK", O.compress2(s, None if table_log == 0 else table_log)[0]
    except O.OracleError as e:
        return e.code, b""


def oracle_checkpoints(comp, ckpt, nstates, spb):
    """The checkpoint entries of one block as the oracle's decoder sees them,
    zero-padded to spb entries: bitpos | s0 << 32 | s1 << 48.  None for a
    single-symbol block: the oracle's walk follows the crate's termination,
    which such a block never reaches (build_frame then stores zeros; the GPU
    tests pass the device's own sidecars instead)."""
    try:
        if nstates == 1:
            bp, s0 = O.checkpoints1(comp, ckpt)
            s1 = np.zeros(len(bp), np.uint16)
        else:
            bp, s0, s1 = O.checkpoints2(comp, ckpt)
    except O.OracleError:
        return None
    side = np.zeros(spb, dtype=np.uint64)
    k = min(len(bp), spb)
    side[:k] = bp[:k].astype(np.uint64) | (s0[:k].astype(np.uint64) << 32) | (s1[:k].astype(np.uint64) << 48)
    return side


def build_frame(raw, block_size, ckpt, nstates, table_log=0, sidecars=None):
    """The frame of `raw` by the encoder rule.  sidecars: a uint64 array of
    spb(block_size) entries per block (the zero-filled sidecar array of
    fsehip_compress_blocks), or None: the oracle's checkpoints."""
    raw = np.frombuffer(bytes(raw), dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw
    n_total = len(raw)
    nb = n_blocks_of(n_total, block_size)
    stride = spb_of(block_size, ckpt, nstates)
    directory, records = [], []
    for b in range(nb):
        s = raw[b * block_size: (b + 1) * block_size]
        status, comp = encode_block(s, nstates, table_log)
        spb = spb_of(len(s), ckpt, nstates)
        rec = len(comp) + 8 * spb
        if status == "ALL_ZERO_SYMBOL0":
            directory.append(RLE << 30 | 1)
            records.append(b"\x00")
        elif status == "OK" and rec < len(s):
            if sidecars is not None:
                side = np.asarray(sidecars, dtype=np.uint64)[b * stride: b * stride + spb]
            else:
                side = oracle_checkpoints(comp, ckpt, nstates, spb) if spb else None
                if side is None:
                    side = np.zeros(spb, np.uint64)
            directory.append(FSE << 30 | len(comp))
            records.append(side.astype("<u8").tobytes() + comp)
        else:
            directory.append(RAW << 30 | len(s))
            records.append(s.tobytes())
    return (header(nstates, kernel_class(table_log), block_size, ckpt, n_total)
            + np.asarray(directory, dtype="<u4").tobytes() + b"".join(records))


def split_frame(frame):
    """(info, directory [(type, stored_len)], records [(checkpoints u64 array, bytes)])."""
    frame = bytes(frame)
    if len(frame) < 32 or frame[:4] != MAGIC:
        raise FrameError("not a frame")
    version, nstates, mlog, flags, bs, ckpt, n_total, nb, reserved = struct.unpack("<BBBBIIQII", frame[4:32])
    info = dict(version=version, nstates=nstates, max_table_log=mlog, flags=flags, block_size=bs, ckpt_interval=ckpt,
                n_total=n_total, n_blocks=nb, records_off=32 + 4 * nb)
    if version != 1 or reserved or nb != n_blocks_of(n_total, bs) or len(frame) < 32 + 4 * nb:
        raise FrameError("bad header")
    d = np.frombuffer(frame, dtype="<u4", count=nb, offset=32)
    directory = [(int(e) >> 30, int(e) & 0x3FFFFFFF) for e in d]
    pos = 32 + 4 * nb
    records = []
    for b, (typ, ln) in enumerate(directory):
        nck = 8 * spb_of(raw_len(n_total, bs, b), ckpt, nstates) if typ == FSE and flags & 1 else 0
        if pos + nck + ln > len(frame):
            raise FrameError("record past the frame")
        records.append((np.frombuffer(frame, dtype="<u8", count=nck // 8, offset=pos), frame[pos + nck: pos + nck + ln]))
        pos += nck + ln
    if pos != len(frame):
        raise FrameError("frame length")
    return info, directory, records


def decode_frame(frame):
    info, directory, records = split_frame(frame)
    out = []
    for b, ((typ, ln), (_, data)) in enumerate(zip(directory, records)):
        n = raw_len(info["n_total"], info["block_size"], b)
        if typ == RAW:
            if ln != n:
                raise FrameError("raw length")
            out.append(data)
        elif typ == RLE:
            if ln != 1:
                raise FrameError("rle length")
            out.append(data * n)
        elif typ == FSE:
            if info["nstates"] == 2:
                out.append(O.decompress2(data, raw_len=n))
            else:  # the 1-state decoder stops at the capacity: the block's raw length
                try:
                    got = O.decompress(data, cap=n)
                except O.OracleError as e:
                    if e.code != "SINGLE_SYMBOL":
                        raise
                    # one symbol holds the whole table: every state decodes to it, reading no bits
                    nh, _ = O.header_read(data)
                    got = bytes([list(nh.norm).index(1 << nh.log2)]) * n
                if len(got) != n:
                    raise FrameError("1-state length")
                out.append(got)
        else:
            raise FrameError("type 3")
    return b"".join(out)


# ---------------------------------------------------------------- the corpus
BLOCK = 4096
CKPT = 128


def _two_symbols(n):
    a = np.full(n, 1, dtype=np.uint8)
    a[::1000] = 2  # [1, 2] at 1:1000
    return a


def corpus(tail=1000):
    """Blocks of 4,096 bytes, one of each case of the encoder rule, then a
    `tail`-byte last block (1,000: LUT data, FSE; 1: TOO_SHORT, RAW)."""
    rng = np.random.default_rng(0xF5EF)
    parts = [
        O.generate(0, 0.155, 0x5EED0002, 0, BLOCK),             # LUT p = 0.155: FSE
        rng.integers(0, 64, BLOCK, dtype=np.uint8),             # uniform 0..63: FSE
        rng.integers(0, 256, BLOCK, dtype=np.uint8),            # uniform 0..255: RAW
        O.generate(2, 0.0, 0x5EED0003, 3, BLOCK),               # uniform 0..239: RAW
        np.zeros(BLOCK, dtype=np.uint8),                        # all zeros: RLE
        np.full(BLOCK, 9, dtype=np.uint8),                      # all 9: FSE (single symbol)
        _two_symbols(BLOCK),                                    # [1, 2] at 1:1000: FSE
        np.concatenate([np.zeros(200, np.uint8), rng.integers(0, 256, BLOCK - 200, dtype=np.uint8)]),  # RAW
        O.generate(0, 0.155, 0x5EED0002, 8, tail),              # the tail
    ]
    return np.concatenate(parts)


def types_of(frame):
    return [t for t, _ in split_frame(frame)[1]]
