/*
 * fsehip.h -- C ABI of the MI355X-native FSE (tANS) entropy coder.
 *
 * Drop-in boundary for the hot path of Cognoscan/entropy_coders (a Rust
 * crate).  Two layers:
 *
 *  (1) Reference-shaped entry points (host pointers, one block per call),
 *      one per public function of the crate on this path.  They keep the
 *      crate's argument meaning and its "append to dst" convention; Rust
 *      panics / None / Err become negative status codes (fse_status.h).
 *      Compute runs on the GPU; there is no CPU fallback.  These are what a
 *      Rust FFI shim binds.
 *
 *  (2) Batched device entry points (fsehip_*): all pointers are device
 *      pointers, calls are asynchronous on `stream` and report a status per
 *      block.  This is the throughput path (bench.py, multi-GPU sharding).
 *
 * Every compressed block is byte-identical to the crate's fse_compress2
 * output for the same input (lib.rs:146-183).
 */
#ifndef FSEHIP_H
#define FSEHIP_H

#include <stddef.h>
#include <stdint.h>

#include "fse_status.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fsehip_stream_t; /* hipStream_t; NULL = the null stream */

/* ------------------------------------------------------------------------
 * (1) Reference-shaped entry points
 * ------------------------------------------------------------------------ */

/* Replaces `pub fn fse_compress2(src: &[u8], dst: &mut Vec<u8>) -> usize`
 * (lib.rs:146).  Appends header||payload at dst[*dst_len], advances
 * *dst_len, and stores the Rust return value (payload bits incl. marker) in
 * *payload_bits.  Errors: EMPTY, TOO_SHORT, ALL_ZERO_SYMBOL0 (reference
 * panics), DST_TOO_SMALL (the reference grows its Vec), UNSUPPORTED (n >
 * 2^28), ENCODER_INIT (the tableLog-15 panic of new_first_symbol). */
int fse_compress2(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len,
                  uint64_t* payload_bits);

/* `Histogram::new(src).normalize(table_log)` followed by the fse_compress2
 * body (histogram.rs:95 + lib.rs:149-182): the tableLog sweep entry point.
 * table_log is clamped to 5..15 as normalize does (0 acts as 5). */
int fse_compress2_log(const uint8_t* src, size_t n, uint32_t table_log, uint8_t* dst, size_t dst_cap,
                      size_t* dst_len, uint64_t* payload_bits);

/* Replaces `pub fn fse_decompress2(src: &[u8], dst: &mut Vec<u8>)
 * -> Option<usize>` (lib.rs:215).  Appends the decoded bytes at
 * dst[*dst_len] and advances *dst_len.  None -> BAD_HEADER / NO_MARKER;
 * the state-read panic -> TOO_SHORT; the never-terminating single-symbol
 * case -> SINGLE_SYMBOL; output beyond dst_cap -> DST_TOO_SMALL (the
 * reference grows its Vec).
 *
 * The host entry points of this section are synchronous on the default
 * stream and stage through per-thread buffers the library keeps: pinned host
 * memory (the input, and up to 4 MiB of the result; larger results come back
 * by a plain device-to-host copy) and device memory (input, output up to
 * dst_cap - *dst_len, tables).  fsehip_release_workspace frees them.  A lone
 * stream decodes as one serial chain (~1.4 ms per 64 KiB call on MI355X,
 * slower than one host core); many streams belong on fse_decompress2_many
 * (host buffers) or fsehip_decompress_streams (device buffers). */
int fse_decompress2(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len);

/* The 1-state format: replaces `pub fn fse_compress(src, dst) -> (NormHistogram, usize)`
 * (lib.rs:112; the returned NormHistogram is the block's own header) and
 * `pub fn fse_decompress(src, dst) -> Option<usize>` (lib.rs:187), same
 * conventions as the 2-state pair above. */
int fse_compress(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len, uint64_t* payload_bits);
int fse_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len);

/* Many fse_decompress2 / fse_decompress calls in one (lib.rs:215-248 /
 * 187-211 per stream): the drop-in for a caller's loop over many crate
 * streams.  Stream i (srcs[i], src_lens[i] bytes) decodes into
 * dst + i * dst_stride with at most dst_stride bytes; dst_lens[i] = bytes
 * decoded and statuses[i] = its status, as the single call would return it
 * (EMPTY, BAD_HEADER, NO_MARKER, TOO_SHORT, SINGLE_SYMBOL, DST_TOO_SMALL,
 * UNSUPPORTED above 2^28 bytes; a null srcs[i] with src_lens[i] > 0 is
 * BAD_ARG).  Returns FSE_OK when the batch ran (look at statuses), or a
 * call-level error (BAD_ARG, NO_DEVICE, HIP).  Streams up to 4 MiB are
 * batched, grouped by the table log in their header (<= 11, 12, 13..15: each
 * group runs the kernels and decode-table stride of its class, so one large
 * or corrupt log does not move the others), in groups of at most 512 MiB of
 * staging each way and 512 MiB of decode tables; longer streams, a log
 * nibble above 15 (a header the crate rejects) and dst_stride above 128 MiB
 * take the single-stream path one by one.
 *
 * Where the GPU pays.  A lone stream is one serial chain: fse_decompress2
 * takes ~1.4 ms per 64 KiB call on MI355X against ~0.14-0.4 ms on one host
 * core, so the per-call path never beats a CPU core.  This call stages all
 * streams through pinned memory in one copy each way and decodes them as
 * thousands of chains at once (fsehip_decompress_streams): 2.6 ms for 16
 * 64 KiB streams, 3.7 ms for 256, 6.3 ms for 1,000 (9.7 GiB/s), 16.5 ms for
 * 4,000 (14.8 GiB/s), PCIe included, so it beats one host core from ~16
 * streams and 16 cores from ~256 (tools/many_streams.py; bench.py's
 * host_call_latency reports 1,000 streams).  One or two streams take the
 * single-stream path; batches of up to 32 streams at table log <= 11 run
 * the single-stream kernel once per stream in one launch (3 streams 1.5 ms,
 * 16 streams 2.1 ms; 1-state 16 streams 2.0 ms, tools/many_ab.py).
 * Synchronous on the default stream; the staging buffers are per thread
 * (grow-only, freed by fsehip_release_workspace). */
int fse_decompress2_many(const uint8_t* const* srcs, const size_t* src_lens, size_t n_streams, uint8_t* dst,
                         size_t dst_stride, size_t* dst_lens, int32_t* statuses);
int fse_decompress_many(const uint8_t* const* srcs, const size_t* src_lens, size_t n_streams, uint8_t* dst,
                        size_t dst_stride, size_t* dst_lens, int32_t* statuses);

/* Many fse_compress2 / fse_compress calls in one (lib.rs:146-183 / 112-143
 * per buffer): the drop-in for a caller's loop over many records, columns or
 * messages, and the mirror image of fse_decompress2_many.  Buffer i
 * (srcs[i], src_lens[i] bytes, any lengths) is compressed into
 * dst + i * dst_stride, at most dst_stride bytes (it does not append);
 * dst_lens[i], payload_bits[i] (may be NULL) and statuses[i] are what
 * fse_compress2(srcs[i], ...) gives into an empty buffer of dst_stride bytes:
 * EMPTY for a zero length, TOO_SHORT, ALL_ZERO_SYMBOL0, UNSUPPORTED above
 * 2^28 bytes, BAD_ARG for a null srcs[i] with a non-zero length, and
 * DST_TOO_SMALL exactly when the compressed length exceeds dst_stride (the
 * device compresses into worst-case regions, so the length is always known);
 * dst_lens[i] = 0 for every failed buffer, and no byte of dst outside a
 * buffer's own first dst_lens[i] bytes is written.  Returns FSE_OK when the
 * batch ran (look at statuses), or a call-level error (BAD_ARG: a null array
 * or dst_stride == 0; UNSUPPORTED: more than 2^24 buffers; NO_DEVICE, HIP).
 *
 * The inputs are packed back to back (16-byte aligned, no common stride: one
 * long buffer does not multiply the staging of the short ones) with their
 * descriptors in pinned memory and go to the device in one copy;
 * fsehip_compress_streams encodes one buffer per wave; the results are
 * compacted on the device, so the copy back carries the compressed bytes
 * (each rounded up to 16) and 12 bytes per buffer, not the capacities.  Calls
 * are split into batches of at most 512 MiB of staging each way; where the
 * split falls does not show in the results.  Synchronous on the default
 * stream; staging buffers per thread (grow-only, fsehip_release_workspace).
 *
 * Where the GPU pays (MI355X, 64 KiB C2 buffers, host buffers in and out,
 * PCIe included; tools/many_compress.py, profiles/many_compress/): 0.212 ms
 * for 2 buffers, 0.218 for 3, 0.272 for 16, 1.41 for 256, 4.09 for 1,000
 * (14.9 GiB/s), 14.1 for 4,000 (17.4 GiB/s); 1,000 buffers of 4 KiB 0.41 ms,
 * 16,000 4.04 ms -- against 0.17-0.19 ms per buffer for a loop of
 * fse_compress2 calls (55 us at 4 KiB) and 0.41 ms per buffer on one host
 * core.  Crossover: the batch wins from two buffers on (0.212 against 0.352
 * ms); one buffer through the batch costs 0.209 ms against the single call's
 * 0.185, so a call of one buffer takes the single call's path. */
int fse_compress2_many(const uint8_t* const* srcs, const size_t* src_lens, size_t n_streams, uint8_t* dst,
                       size_t dst_stride, size_t* dst_lens, uint64_t* payload_bits, int32_t* statuses);
int fse_compress_many(const uint8_t* const* srcs, const size_t* src_lens, size_t n_streams, uint8_t* dst,
                      size_t dst_stride, size_t* dst_lens, uint64_t* payload_bits, int32_t* statuses);

/* Replaces `Histogram::new(data)` (histogram.rs:18-66) -- the north star's
 * `histogram::count`: counts[256], table_len = 1 + largest symbol. */
int histogram_count(const uint8_t* src, size_t n, uint32_t counts[256], uint32_t* table_len);

/* ------------------------------------------------------------------------
 * (1b) The crate's building blocks, as plain-data structs (repr(C) twins of
 * the Rust types; every table has room for the largest log, 15) and calls
 * that run on the GPU.  Same argument meaning and panics-as-statuses as
 * above; host pointers.
 * ------------------------------------------------------------------------ */

/* Histogram (histogram.rs:9-14): counts, size = input length, table_len =
 * 1 + the largest symbol (1 when empty). */
typedef struct {
    uint32_t counts[256];
    uint32_t size;
    uint32_t table_len;
} fse_histogram;

/* NormHistogram (histogram.rs:289-294): norm[s] in {-1, 0, 1..2^log2}. */
typedef struct {
    int32_t norm[256];
    uint32_t log2;
    uint32_t table_len;
} fse_norm_histogram;

/* EncodeTable (fse.rs:72-84): stateTable (`table`, 2^table_log used),
 * the spread (`symbols`) and the symbol transforms. */
typedef struct {
    uint32_t bits;      /* deltaNbBits */
    int32_t find_state; /* deltaFindState */
} fse_symbol_transform;
typedef struct {
    uint32_t table_log;
    uint16_t table[1u << 15];
    uint8_t symbols[1u << 15];
    fse_symbol_transform symbol_tt[256];
} fse_encode_table;

/* DecodeTable (fse.rs:253-265). */
typedef struct {
    uint16_t new_state;
    uint8_t symbol;
    uint8_t num_bits;
} fse_decode_transform;
typedef struct {
    uint32_t table_log;
    uint32_t fast_mode; /* no symbol with norm >= 2^(table_log-1) (fse.rs:302-305) */
    fse_decode_transform table[1u << 15];
} fse_decode_table;

/* Histogram::new (histogram.rs:18-66). */
int histogram_new(const uint8_t* src, size_t n, fse_histogram* out);
/* Histogram::normalize(log2) (histogram.rs:95-155): log2 is clamped to 5..15
 * and raised to ilog2(table_len - 1) + 2 as in the reference. */
int histogram_normalize(const fse_histogram* h, uint32_t log2, fse_norm_histogram* out);
/* Histogram::normalize_optimal (histogram.rs:281-284, optimal_log2 264-277). */
int histogram_normalize_optimal(const fse_histogram* h, fse_norm_histogram* out);
/* NormHistogram::new (histogram.rs:299-303). */
int norm_histogram_new(const uint8_t* src, size_t n, fse_norm_histogram* out);
/* NormHistogram::write (histogram.rs:376-431): appends the header at
 * dst[*dst_len], advances *dst_len, *bits_written = the returned bit count. */
int norm_histogram_write(const fse_norm_histogram* nh, uint8_t* dst, size_t dst_cap, size_t* dst_len,
                         uint64_t* bits_written);
/* NormHistogram::read (histogram.rs:436-505): *consumed = header bytes (the
 * remaining slice starts there).  Errors: BAD_HEADER (TableLogTooLarge,
 * TooManySymbols, UnexpectedEof), EMPTY. */
int norm_histogram_read(const uint8_t* src, size_t n, fse_norm_histogram* out, size_t* consumed);
/* EncodeTable::new / DecodeTable::new (fse.rs:88-189, 269-338). */
int encode_table_new(const fse_norm_histogram* nh, fse_encode_table* out);
int decode_table_new(const fse_norm_histogram* nh, fse_decode_table* out);
/* fse_compress with its returned NormHistogram (lib.rs:112: the tuple's
 * first element); otherwise as fse_compress. */
int fse_compress_nh(const uint8_t* src, size_t n, uint8_t* dst, size_t dst_cap, size_t* dst_len,
                    uint64_t* payload_bits, fse_norm_histogram* nh);

/* The bitstream (bitstream/mod.rs:9-15).  A field is (value, width), width
 * <= 32 (the crate's writer and readers take <= 16).
 *  bitstack_write: BitStackWriter::new(dst) + write_bits_unmasked(vals[i],
 *    nbits[i]) for each field + finish() (writer.rs:14-222): the fields
 *    LSB-first from byte *dst_len on, zero-padded to a byte; appends,
 *    advances *dst_len, *bits_written = finish()'s count.
 *  bitstack_read: BitStackReader::new(src) (None -> NO_MARKER: empty or a
 *    zero last byte, stack_reader.rs:17-92) + read(nbits[i]) per field
 *    (top down); *n_read = reads that returned Some (the first None stops
 *    them), *finished = finish() after them (stack_reader.rs:224-226).
 *  bitstream_read: BitStreamReader::new(src, total_bits) (asserts
 *    n == ceil(total_bits / 8) > 0 -> BAD_ARG) + read(nbits[i]) per field;
 *    *n_read = reads that returned Ok, *bits_left = available() after them. */
int bitstack_write(const uint32_t* vals, const uint8_t* nbits, size_t count, uint8_t* dst, size_t dst_cap,
                   size_t* dst_len, uint64_t* bits_written);
int bitstack_read(const uint8_t* src, size_t n, const uint8_t* nbits, size_t count, uint32_t* vals, size_t* n_read,
                  int* finished);
int bitstream_read(const uint8_t* src, size_t n, uint64_t total_bits, const uint8_t* nbits, size_t count,
                   uint32_t* vals, size_t* n_read, uint64_t* bits_left);
/* BitStreamReader with each field's call named (stream_reader.rs:56-119):
 * ops[i] = FSE_BITS_READ (read), FSE_BITS_PEEK (peek: value, no advance) or
 * FSE_BITS_ADVANCE (advance_by: advance, value 0).  Any of them fails past
 * total_bits (UnexpectedEof) and stops the list: *n_done = steps that
 * returned Ok, *bits_left = available() after them (finish(): the remaining
 * slice starts at byte (total_bits - *bits_left) / 8, finish_byte() at the
 * next byte boundary).  ops = NULL: all reads, as bitstream_read. */
#define FSE_BITS_READ 0
#define FSE_BITS_PEEK 1
#define FSE_BITS_ADVANCE 2
int bitstream_read_ops(const uint8_t* src, size_t n, uint64_t total_bits, const uint8_t* nbits, const uint8_t* ops,
                       size_t count, uint32_t* vals, size_t* n_done, uint64_t* bits_left);

/* ------------------------------------------------------------------------
 * (1c) The bit readers and writer as incremental cursors
 *
 * The crate's callers drive its readers one field at a time with widths
 * chosen from earlier values (NormHistogram::read, histogram.rs:453-496; the
 * decoders, fse.rs:349-385).  Each reader / writer is a plain struct the
 * caller owns (no allocation, no handle table) and every call is O(1):
 * a Rust shim wraps it as BitStackReader / BitStreamReader / BitStackWriter
 * with the same method names.  These run on the
 * caller's side of the ABI (host): one field is a few shifts.  Millions of
 * fields with known widths go through the batched device forms
 * (fsehip_bitstack_write / fsehip_bitstack_read / fsehip_bitstream_read_ops).
 * Semantics are the crate's on a 64-bit target (32-bit refills/flushes),
 * including available(), which depends on the buffer's address alignment as
 * the crate's does.  None / Err(UnexpectedEof) -> FSE_ERR_EOF; the crate's
 * debug assertions (width > 32, advance past the buffer) -> FSE_ERR_BAD_ARG.
 * ------------------------------------------------------------------------ */

/* BitStackReader (stack_reader.rs:5-227): reads the stack from the end,
 * after the marker bit. */
typedef struct {
    const uint8_t* base; /* the slice */
    const uint8_t* ptr;  /* next refill address */
    uint64_t buffer;
    uint64_t bits;       /* bits buffered: available() */
    int32_t finished;
    int32_t reserved;
} fse_bitstack_reader;
/* new (stack_reader.rs:17-92): None (empty slice, zero last byte, marker not
 * in the last byte) -> FSE_ERR_NO_MARKER */
int bitstack_reader_new(fse_bitstack_reader* r, const uint8_t* src, size_t n);
int bitstack_reader_reload(fse_bitstack_reader* r);                                        /* 97-172 */
int bitstack_reader_peek(const fse_bitstack_reader* r, uint32_t nbits, uint32_t* val);      /* 176-184 */
int bitstack_reader_read_no_reload(fse_bitstack_reader* r, uint32_t nbits, uint32_t* val); /* 193-197 */
int bitstack_reader_advance_no_reload(fse_bitstack_reader* r, uint32_t nbits);             /* 204-207 */
int bitstack_reader_read(fse_bitstack_reader* r, uint32_t nbits, uint32_t* val);           /* 211-215 */
uint64_t bitstack_reader_available(const fse_bitstack_reader* r);                          /* 218-220 */
int bitstack_reader_finish(const fse_bitstack_reader* r); /* 224-226: 1 if every bit was read */

/* BitStreamReader (stream_reader.rs:5-136): forward LSB-first reader. */
typedef struct {
    const uint8_t* src;
    uint64_t n;
    uint64_t total_bits;
    uint64_t bits_read;
} fse_bitstream_reader;
/* new (stream_reader.rs:16-49): n == 0 or n != ceil(total_bits/8) (the
 * crate's asserts) -> FSE_ERR_BAD_ARG */
int bitstream_reader_new(fse_bitstream_reader* r, const uint8_t* src, size_t n, uint64_t total_bits);
int bitstream_reader_read(fse_bitstream_reader* r, uint32_t nbits, uint32_t* val);       /* 56-60 */
int bitstream_reader_advance_by(fse_bitstream_reader* r, uint32_t nbits);                /* 67-75 */
int bitstream_reader_peek(const fse_bitstream_reader* r, uint32_t nbits, uint32_t* val); /* 82-114 */
uint64_t bitstream_reader_available(const fse_bitstream_reader* r);                      /* 117-119 */
/* finish (123-128): the remaining slice starts at src + *byte, *remaining
 * bits, *offset bits into its first byte */
int bitstream_reader_finish(const fse_bitstream_reader* r, size_t* byte, uint64_t* remaining, uint32_t* offset);
/* finish_byte (132-135): offset of the remaining bytes (next byte boundary) */
size_t bitstream_reader_finish_byte(const fse_bitstream_reader* r);

/* BitStackWriter (writer.rs:5-223) appending to dst[len..cap).  Whole bytes
 * are committed to dst as they complete; a full buffer is a sticky
 * FSE_ERR_DST_TOO_SMALL (the crate grows its Vec). */
typedef struct {
    uint8_t* dst;
    uint64_t cap;
    uint64_t len;         /* bytes committed (the Vec's length at finish) */
    uint64_t initial_len;
    uint64_t storage;     /* pending bits, LSB-first */
    uint32_t bits;
    int32_t status;
} fse_bitstack_writer;
int bitstack_writer_new(fse_bitstack_writer* w, uint8_t* dst, size_t cap, size_t len); /* 16-40 */
int bitstack_writer_flush(fse_bitstack_writer* w);                                     /* 43-110 */
/* write_bits_raw (164-180): val's bits above nbits must be zero; no flush */
int bitstack_writer_write_bits_raw(fse_bitstack_writer* w, uint32_t val, uint32_t nbits);
int bitstack_writer_write_bits_raw_unmasked(fse_bitstack_writer* w, uint32_t val, uint32_t nbits); /* 140-149 */
int bitstack_writer_write_bits(fse_bitstack_writer* w, uint32_t val, uint32_t nbits);          /* 185-188 */
int bitstack_writer_write_bits_unmasked(fse_bitstack_writer* w, uint32_t val, uint32_t nbits); /* 193-198 */
/* finish (201-222): zero-pads the last byte; *dst_len = new length of dst,
 * *bits_written = bits written since new() */
int bitstack_writer_finish(fse_bitstack_writer* w, size_t* dst_len, uint64_t* bits_written);

/* ------------------------------------------------------------------------
 * (2) Batched device entry points
 * ------------------------------------------------------------------------ */

typedef struct {
    uint32_t block_size;    /* bytes per block, <= 2^28 (u32 bit counts); multiple of 16 when >1 block; default 65536 */
    uint32_t table_log;     /* 0 = NormHistogram::new (optimal); else Histogram::normalize(L) */
    uint32_t ckpt_interval; /* steps between decode checkpoints (power of two; >= 8 for 2-state
                               pairs, >= 16 for 1-state symbols), 0 = none */
    uint32_t max_table_log; /* upper bound on L used by the blocks (5..15; kernels exist for <= 11,
                               12, 13, 14 and 15); 0 = derive (encode) / 12 (decode) */
    uint32_t nstates;       /* block format: 2 (or 0) = fse_compress2 (lib.rs:146), 1 = fse_compress (lib.rs:112) */
} fsehip_params;

/* Per-block output slot size (bytes) able to hold any block of block_size
 * bytes at tableLog <= max_table_log, and sidecar entries per block (2-state
 * blocks; the _ns variant covers both formats). */
uint64_t fsehip_slot_bytes(uint32_t block_size, uint32_t max_table_log);
uint32_t fsehip_sidecar_per_block(uint32_t block_size, uint32_t ckpt_interval);
uint32_t fsehip_sidecar_per_block_ns(uint32_t block_size, uint32_t ckpt_interval, uint32_t nstates);

/* Compress n_total bytes as ceil(n_total/block_size) independent blocks.
 * Block b's bytes go to d_out + b*slot_bytes (comp_len[b] bytes, exactly
 * fse_compress2's output); d_sidecar (optional) receives the decode
 * checkpoints: entry = bitpos(32, payload-relative) | s0<<32 | s1<<48 for
 * the decoder state before pair k*ckpt_interval.  A slot's bytes beyond
 * comp_len[b] are unspecified: at table logs 13..15 the kernels use them
 * as scratch (the spread's 2^L symbols after the first 512 bytes); slots
 * smaller than 512 + 2^L bytes make the call take a workspace buffer of
 * 2^L bytes per block instead (see fsehip_decompress_blocks). */
int fsehip_compress_blocks(const fsehip_params* p, const uint8_t* d_src, uint64_t n_total, uint8_t* d_out,
                           uint64_t slot_bytes, uint32_t* d_comp_len, uint32_t* d_payload_bits,
                           uint64_t* d_sidecar, int32_t* d_status, fsehip_stream_t stream);

/* Decompress blocks produced as above.  With d_sidecar the blocks decode in
 * parallel segments; without it (any valid fse_compress2 stream, e.g. from
 * the CPU crate) each block decodes serially, many at once (one lane per
 * block, its table compact in LDS).  Blocks at table log <= 11 (both formats) keep
 * only the u16 table entries in LDS (8 blocks per workgroup, 32 chains per
 * CU) and defer their symbols: the chains write state pairs into the
 * stream's workspace and a map kernel turns them into bytes; if that
 * workspace cannot be allocated (or the batch has 2^24 blocks or more), the
 * single-kernel decode runs (6 blocks per workgroup, 24 chains per CU).
 * n_total (> 0) gives the raw length.  slot_bytes is a multiple of 256, as
 * encoder slots are (the decode-table build requires it); d_in and d_out
 * 16-byte aligned (BAD_ARG otherwise).
 *
 * Workspace (device memory owned by the library, one per (device, stream),
 * grown on demand and kept for reuse until fsehip_release_workspace):
 *   decode tables  fsehip_dtable_bytes(max_table_log) + 4 bytes per block
 *                  (every call of fsehip_decompress_blocks / _streams /
 *                  fsehip_build_sidecar);
 *   deferred symbols (sidecar-less decode at table log <= 11 only):
 *                  2 bytes per output byte of the batch's capacity
 *                  (n_blocks x block_size) + 8 bytes per block -- 2 GiB for a
 *                  1 GiB batch.  A size that failed to allocate is remembered
 *                  (later calls of that size or more take the single-kernel
 *                  decode without retrying) until the next release;
 *   encode spread  2^L bytes per block (L the encode kernel's table log,
 *                  13..15) when the slots are smaller than 512 + 2^L bytes
 *                  (fsehip_compress_blocks), and always 2^L bytes per stream
 *                  in fsehip_compress_streams (a stream's output region is
 *                  never scratch);
 *   header parse   520 bytes per block (the headers parsed one per lane
 *                  before the table build: batches of >= 256 blocks at
 *                  max_table_log <= 12, fsehip_build_dtables included;
 *                  without it the tables kernel parses on its own);
 *   frame chunk    (fsehip_frame_compress / fsehip_frame_decompress, per chunk
 *                  of chunk_blocks blocks, whatever n_total is)
 *                  chunk_blocks * slot_bytes          the chunk's slots,
 *                  (12 + 8 * spb) * chunk_blocks      comp_len, status, record
 *                                                     type and checkpoints
 *                                                     (spb entries per block),
 *                  8 * chunk_blocks + 8               record offsets and the
 *                                                     running frame offset,
 *                  plus the encode-spread / decode-table / deferred-symbol
 *                  entries above for a batch of chunk_blocks blocks;
 *   frame ranges   (fsehip_frame_decompress_ranges) the frame chunk entries
 *                  above for the largest chunk the call runs (at most
 *                  chunk_blocks blocks), plus
 *                  chunk * block_size                 the bounce chunk's
 *                                                     decoded blocks,
 *                  8 per listed block                 record offsets (the
 *                                                     seek pass keeps the
 *                                                     covered blocks' only,
 *                                                     not one per block of
 *                                                     the frame),
 *                  16 per listed block, 4 per bounced block, 24 per bounce
 *                  piece, 8 per range + 8             block number, record
 *                                                     type, comp_len, status
 *                                                     and the planner's
 *                                                     lists,
 *                  and pinned host staging for the lists (64 KiB a buffer, or
 *                  the next power of two that holds them).
 * Growing a buffer synchronises the stream before freeing the old one.
 * First table build on a device (any encode or decode call): the library
 * first runs a ~1 ms synchronous self-check on the null stream (the lane
 * order of same-address LDS atomics that its rank pass relies on; the
 * slower peer-mask ranks are used if it fails), so issue one call before
 * capturing a stream into a graph. */
int fsehip_decompress_blocks(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes,
                             const uint32_t* d_comp_len, const uint64_t* d_sidecar, uint8_t* d_out,
                             uint64_t n_total, int32_t* d_status, fsehip_stream_t stream);

/* Decode tables, built once per block (NormHistogram::read + DecodeTable,
 * histogram.rs:436-505, fse.rs:280-338) for decode-only workloads (C3):
 * d_dtables holds fsehip_dtable_bytes(max_table_log) bytes per block (entry
 * u32 = nbBits | symbol << 8 | newState << 18 for max_table_log <= 14, and
 * newState << 17 at 15), d_dtinfo one int32 per
 * block (header bytes | tableLog << 16, or a negative status).
 * The tables go to the caller's buffers, but a batch of >= 256 blocks at
 * max_table_log <= 12 first parses its headers into the stream's workspace
 * (520 bytes per block, the header-parse entry of the workspace note at
 * fsehip_decompress_blocks): the call then holds that workspace's lock, so
 * it is serialised with the library's other calls on the same stream, and
 * growing the scratch synchronises the stream (the host blocks until the
 * stream's earlier work is done).  fsehip_release_workspace frees it. */
uint64_t fsehip_dtable_bytes(uint32_t max_table_log);
int fsehip_build_dtables(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes,
                         const uint32_t* d_comp_len, uint32_t n_blocks, uint32_t* d_dtables, int32_t* d_dtinfo,
                         fsehip_stream_t stream);
/* Decompress with prebuilt tables, with or without the sidecar (as above;
 * here slot_bytes need only be a multiple of 32, the staging loads' chunk).
 * fsehip_build_dtables requires a multiple of 256.
 * fsehip_decompress_blocks runs fsehip_build_dtables + this into a
 * per-stream workspace. */
int fsehip_decompress_blocks_dt(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes,
                                const uint32_t* d_comp_len, const uint64_t* d_sidecar, const uint32_t* d_dtables,
                                const int32_t* d_dtinfo, uint8_t* d_out, uint64_t n_total, int32_t* d_status,
                                fsehip_stream_t stream);

/* Serial decode that also records the sidecar index (for streams produced
 * elsewhere, e.g. by the CPU crate), so later decodes run in parallel.
 * 1-state blocks: table logs <= 12 (UNSUPPORTED above). */
int fsehip_build_sidecar(const fsehip_params* p, const uint8_t* d_in, uint64_t slot_bytes,
                         const uint32_t* d_comp_len, uint8_t* d_out, uint64_t n_total, uint64_t* d_sidecar_out,
                         int32_t* d_status, fsehip_stream_t stream);

/* Batched fse_decompress2 / fse_decompress (nstates 2 / 1) in the crate's
 * own termination (lib.rs:215-248 / 187-211), for streams with no sidecar
 * and no recorded raw length, e.g. many outputs of the CPU crate.  Stream b:
 * d_comp_len[b] bytes at d_in + b * in_stride (in_stride a multiple of 256
 * and at least the largest stream; d_in 16-byte aligned); its output at d_out + b *
 * out_stride, at most out_stride bytes; d_out_len[b] = bytes decoded.
 * d_status[b]: DST_TOO_SMALL when out_stride is short, SINGLE_SYMBOL for a
 * stream the crate would decode forever, UNSUPPORTED for a table log above
 * the kernels' bound or a stream above 2^28 bytes.  The bound is
 * max_table_log (0 = 11; below 11 it is 11: the smallest kernel variant);
 * the decode-table workspace is 4 << bound bytes per stream (8 KiB at 11,
 * 16 KiB at 12, 32 / 64 / 128 KiB at 13 / 14 / 15), plus 2 * out_stride + 8
 * bytes per stream for the deferred symbols of streams at bound 11 (sized by
 * the capacity out_stride, not by the bytes decoded; see the workspace note
 * at fsehip_decompress_blocks and fsehip_release_workspace).
 * out_stride must be a multiple of 16 and d_out 16-byte aligned (the decoder
 * stores 16-byte groups; BAD_ARG otherwise).
 * Serial per stream, many streams at once. */
int fsehip_decompress_streams(uint32_t nstates, uint32_t max_table_log, const uint8_t* d_in, uint64_t in_stride,
                              const uint32_t* d_comp_len, uint32_t n_streams, uint8_t* d_out, uint32_t out_stride,
                              uint32_t* d_out_len, int32_t* d_status, fsehip_stream_t stream);

/* Batched fse_compress2 / fse_compress (nstates 2 or 0 / 1) of n_streams
 * independent inputs of any lengths: the compress side of
 * fsehip_decompress_streams.  Stream i is the src_len bytes at
 * d_src + src_off; its header||payload goes to d_out + out_off, at most
 * out_cap bytes, and is byte for byte what fse_compress2 / fse_compress
 * produce for that input -- with table_log != 0 what fse_compress2_log does
 * (Histogram::normalize(table_log), clamped to 5..15); table_log 0 picks
 * each stream's own optimal_log2.  max_table_log bounds the table log of the
 * kernels as in fsehip_params (0 = derive: 11, or table_log above it).
 *
 * d_comp_len[i], d_payload_bits[i] (may be NULL) and d_status[i] are the
 * single call's: EMPTY, TOO_SHORT, ALL_ZERO_SYMBOL0, CURSED, BAD_TABLE and
 * ENCODER_INIT in the same cases; UNSUPPORTED for src_len above 2^28 or a
 * table log above the kernel bound; DST_TOO_SMALL when the stream does not
 * fit out_cap; BAD_ARG when src_off or out_off is not a multiple of 16.
 * d_comp_len[i] = 0 for every stream that failed.
 *
 * Memory rules.  Reads: exactly [src_off, src_off + src_len) of each stream
 * (16-byte loads only where a whole aligned chunk lies inside the stream, the
 * rest bytewise), so nothing past src_len need be readable; d_src itself
 * 16-byte aligned.  Stores: only inside [out_off, out_off + out_cap), whatever
 * the status (a region too small for the header stays untouched; bytes of a
 * region beyond d_comp_len[i] are unspecified); d_out 16-byte aligned.
 * Regions must not overlap.  fsehip_stream_out_bytes(src_len, max_table_log)
 * is a capacity that always suffices.  There is no sidecar: the streams
 * decode with fsehip_decompress_streams.
 *
 * Workspace: at kernel table logs 13..15 the spread's 2^L-byte symbol array
 * of every stream is leased from the stream's workspace (n_streams << L
 * bytes, the encode-spread entry of the workspace note at
 * fsehip_decompress_blocks) -- a stream's output region is never used as
 * scratch, whatever its capacity.
 *
 * Asynchronous on `stream`.  n_streams == 0 returns FSE_OK and does
 * nothing; a null pointer, nstates > 2 or a misaligned d_src / d_out is
 * BAD_ARG, n_streams > 2^24 or max_table_log > 15 UNSUPPORTED, before any
 * device use; otherwise NO_DEVICE or HIP. */
typedef struct {
    uint64_t src_off; /* byte offset of the stream in d_src, a multiple of 16 */
    uint64_t out_off; /* byte offset of its output region in d_out, a multiple of 16 */
    uint32_t src_len; /* bytes, <= 2^28 */
    uint32_t out_cap; /* bytes of the output region (any value) */
} fsehip_stream_desc;
int fsehip_compress_streams(uint32_t nstates, uint32_t table_log, uint32_t max_table_log, const uint8_t* d_src,
                            const fsehip_stream_desc* d_desc, uint32_t n_streams, uint8_t* d_out,
                            uint32_t* d_comp_len, uint32_t* d_payload_bits, int32_t* d_status,
                            fsehip_stream_t stream);
/* Output capacity that holds any stream of src_len bytes at table logs <=
 * max_table_log (0 = 12): 512 header bytes + src_len * L + 2 L + 1 bits,
 * rounded up to 16 bytes. */
uint64_t fsehip_stream_out_bytes(uint32_t src_len, uint32_t max_table_log);

/* Free the workspace of (device, stream) -- device < 0: of every device for
 * that stream handle -- after the work already enqueued on the stream, plus
 * the calling thread's staging buffers of the host entry points.  The next
 * call allocates again.  Call it before destroying a stream the library has
 * been used on.  Returns FSE_OK, or HIP if a synchronise / free failed. */
int fsehip_release_workspace(int device, fsehip_stream_t stream);

/* Compact the slot layout into one stream (blocks back to back at the byte
 * offsets d_offsets[b], an exclusive scan of d_comp_len) and back.  Used to
 * ship compressed shards between GPUs (RCCL gather) or to the host.
 * Block b is the first d_comp_len[b] bytes of the slot at d_slots +
 * b * slot_bytes (slot_bytes a multiple of 16; d_slots and d_stream 4-byte
 * aligned, as device allocations are).
 *  fsehip_pack_blocks stores exactly the bytes [d_offsets[b], d_offsets[b] +
 *    d_comp_len[b]) of d_stream, whatever their alignment (a dword shared by
 *    two blocks is written bytewise by each), and reads each slot in whole
 *    dwords: up to roundup(d_comp_len[b], 4) bytes of it, never more.
 *  fsehip_unpack_blocks stores exactly the first d_comp_len[b] bytes of each
 *    slot (the rest of the slot keeps what it held) and reads exactly the
 *    block's bytes of d_stream.
 * n_blocks == 0 returns FSE_OK and does nothing. */

int fsehip_pack_blocks(const uint8_t* d_slots, uint64_t slot_bytes, const uint32_t* d_comp_len,
                       const uint64_t* d_offsets, uint32_t n_blocks, uint8_t* d_stream, fsehip_stream_t stream);
int fsehip_unpack_blocks(const uint8_t* d_stream, const uint64_t* d_offsets, const uint32_t* d_comp_len,
                         uint32_t n_blocks, uint8_t* d_slots, uint64_t slot_bytes, fsehip_stream_t stream);

/* Move whole blocks between packed streams: block b's d_lens[b] bytes go from
 * d_src + d_src_offsets[b] to d_dst + d_dst_offsets[b] (any byte offsets;
 * ranges must not overlap).  Selects one rank's blocks out of a packed
 * stream for the distributed scatter (entropy_coders_amd/dist.py).
 * d_src and d_dst themselves may have any alignment as well: the kernel
 * counts its dwords from them, and global memory on gfx950 takes the
 * unaligned dword accesses this gives.  Stores: exactly the bytes of each
 * destination range (a dword shared by two blocks is written bytewise by
 * each).  Reads: the whole dwords, counted from d_src, that hold a byte of
 * the block: never below d_src, and at most up to d_src +
 * roundup(d_src_offsets[b] + d_lens[b], 4), which must be readable.
 * n_blocks == 0 returns FSE_OK and does nothing. */
int fsehip_copy_blocks(const uint8_t* d_src, const uint64_t* d_src_offsets, const uint32_t* d_lens, uint32_t n_blocks,
                       uint8_t* d_dst, const uint64_t* d_dst_offsets, fsehip_stream_t stream);

/* ------------------------------------------------------------------------
 * (2b) The frame: one self-describing buffer for any input
 *
 * This library's own container around the crate-exact blocks (it is not a
 * crate format).  compress(anything) gives one buffer that decodes from its
 * bytes alone, never expands beyond fsehip_frame_bound, and round-trips the
 * inputs the block codec refuses (all zeros, a 1-byte tail, the crate's
 * panics, an empty input).  Version 1; integers little-endian, no padding,
 * a frame may start at any byte address:
 *
 *   header, 32 bytes
 *      0  u8[4] magic "FSEF"
 *      4  u8    version = 1
 *      5  u8    nstates (1 or 2)
 *      6  u8    max_table_log  kernel class the blocks were encoded under (11..15)
 *      7  u8    flags          bit 0: records carry decode checkpoints; others 0
 *      8  u32   block_size     1..2^28; a multiple of 16 when n_blocks > 1
 *     12  u32   ckpt_interval  0 when flags bit 0 is clear; else a power of two,
 *                              >= 8 (2-state) / >= 16 (1-state)
 *     16  u64   n_total        raw bytes
 *     24  u32   n_blocks       = ceil(n_total / block_size); 0 for an empty input
 *     28  u32   reserved = 0
 *   directory, n_blocks x u32: type << 30 | stored_len
 *      type 0 RAW  stored_len = raw_len_b  the block's bytes as they are
 *      type 1 RLE  stored_len = 1          one byte, repeated raw_len_b times
 *      type 2 FSE  stored_len = comp_len   the crate-exact header||payload
 *      type 3 invalid
 *   records, back to back in block order from byte 32 + 4 * n_blocks
 *      RAW / RLE: stored_len bytes
 *      FSE: [spb_b x u64 checkpoints, when flags bit 0] then stored_len bytes
 *
 * raw_len_b = min(block_size, n_total - b * block_size); spb_b =
 * fsehip_sidecar_per_block_ns(raw_len_b, ckpt_interval, nstates); the
 * checkpoints are the entries fsehip_compress_blocks writes for the block
 * into a zero-filled sidecar (entries it leaves unwritten are zero).  The
 * frame ends with its last record; a decoder rejects any other length.
 *
 * Encoder rule (frames are deterministic): with rec = comp_len + 8 * spb_b
 * (comp_len alone without checkpoints), block b is RLE of byte 0 iff its
 * encode status is ALL_ZERO_SYMBOL0, FSE iff the status is FSE_OK and
 * rec < raw_len_b, RAW otherwise (every other status, every block that would
 * not shrink).  Hence frame_len <= 32 + 4 * n_blocks + n_total.  A decoder
 * accepts RLE of any byte.
 * ------------------------------------------------------------------------ */

/* The header's fields, plus records_off = 32 + 4 * n_blocks. */
typedef struct {
    uint32_t version, nstates, max_table_log, flags;
    uint32_t block_size, ckpt_interval, n_blocks, reserved;
    uint64_t n_total, records_off;
} fsehip_frame_info;

/* 32 + 4 * ceil(n_total / block_size) + n_total (block_size 0 = 65536): a
 * capacity no frame of n_total bytes exceeds. */
uint64_t fsehip_frame_bound(uint64_t n_total, uint32_t block_size);
/* Parse and validate the first 32 bytes of a frame (host pointer; len = bytes
 * available, only the first 32 are read).  FSE_ERR_BAD_FRAME for len < 32,
 * bad magic / version / field, a nonzero reserved word or flag bit, or
 * n_blocks != ceil(n_total / block_size). */
int fsehip_frame_read_header(const uint8_t* hdr, size_t len, fsehip_frame_info* out);
/* The 32 header bytes of `info` (records_off is not stored); BAD_ARG when
 * the fields would not pass fsehip_frame_read_header. */
int fsehip_frame_write_header(const fsehip_frame_info* info, uint8_t hdr[32]);

typedef struct {
    uint32_t block_size, table_log, ckpt_interval, max_table_log, nstates; /* as fsehip_params */
    uint32_t chunk_blocks; /* blocks encoded per pass; 0 = 4096 */
} fsehip_frame_params;

/* Compress n_total bytes (0 is valid: a 32-byte frame) into one frame at
 * d_frame (any byte alignment; frame_cap >= fsehip_frame_bound, else
 * DST_TOO_SMALL).  *d_frame_len = the frame's length, d_result[0] = frame
 * status (FSE_OK), d_result[1] = blocks not stored as FSE.  Only the first
 * *d_frame_len bytes of d_frame are written.  d_src 16-byte aligned; RAW
 * blocks are copied from it in 16-byte or aligned 4-byte reads, so up to
 * roundup(n_total, 4) bytes of it are read.
 *
 * Works in chunks of chunk_blocks blocks (fewer when chunk_blocks slots would
 * exceed 1 GiB), so the workspace is bounded whatever n_total is (the frame
 * entries of the workspace note at fsehip_decompress_blocks); where the split
 * falls does not show in the frame.  Per chunk: the batch encoder into slot
 * scratch, a plan kernel (encoder rule, directory, record offsets), a pack
 * kernel (one workgroup per block).
 *
 * Asynchronous on `stream`, no host synchronisation except when the
 * workspace grows.  Before any device use: BAD_ARG (null pointer, nstates >
 * 2, a bad ckpt_interval, block_size not a multiple of 16 with more than one
 * block, d_src not 16-byte aligned), UNSUPPORTED (block_size > 2^28),
 * DST_TOO_SMALL, NO_DEVICE. */
int fsehip_frame_compress(const fsehip_frame_params* p, const uint8_t* d_src, uint64_t n_total, uint8_t* d_frame,
                          uint64_t frame_cap, uint64_t* d_frame_len, int32_t* d_result, fsehip_stream_t stream);

/* Decompress the frame of frame_len bytes at d_frame (any alignment) whose
 * header fsehip_frame_read_header parsed into `info` (the caller copies the
 * 32 bytes to the host).  d_out: info->n_total bytes (out_cap >= n_total,
 * else DST_TOO_SMALL), 16-byte aligned.  d_block_status (n_blocks entries,
 * may be NULL): FSE_OK, the block decoder's status for an FSE block, or
 * BAD_FRAME for a bad directory entry (type 3, a RAW length other than
 * raw_len_b, an RLE length other than 1, an FSE length of 0 or above
 * fsehip_slot_bytes(block_size, max_table_log)); such a block alone is
 * skipped.  d_result[0] = frame status, d_result[1] = failed blocks.
 *
 * Before anything is copied a kernel checks that the header on the device
 * equals `info` and that the directory's record lengths (stored_len, plus
 * the checkpoints of a type-2 entry) end exactly at frame_len; so every
 * offset a copy uses lies inside the frame.  A frame that fails this gets
 * d_result[0] = BAD_FRAME, every block status BAD_FRAME, and no byte of
 * d_out is touched.  Reads of d_frame: its bytes, in 16-byte or aligned
 * 4-byte accesses that hold at least one byte of the frame.
 *
 * Chunked as the compress side (chunk_blocks 0 = 4096): records are
 * scattered into slot scratch (RAW copied, RLE filled straight into d_out),
 * then the table build and decode of fsehip_decompress_blocks run on the
 * chunk -- segment-parallel with checkpoints, serial without.  Asynchronous;
 * call-level errors as fsehip_frame_compress (BAD_ARG also for an `info`
 * that fsehip_frame_read_header would reject or a misaligned d_out). */
int fsehip_frame_decompress(const fsehip_frame_info* info, uint32_t chunk_blocks, const uint8_t* d_frame,
                            uint64_t frame_len, uint8_t* d_out, uint64_t out_cap, int32_t* d_block_status,
                            int32_t* d_result, fsehip_stream_t stream);

/* One byte range of a frame's raw content and where it goes. */
typedef struct {
    uint64_t src_off; /* first raw byte of the range */
    uint64_t len;     /* bytes; 0 is valid */
    uint64_t dst_off; /* the range goes to d_out + dst_off */
} fsehip_frame_range;

/* Decode byte ranges of a frame without decoding the rest of it: range r's
 * bytes [src_off, src_off + len) of the raw content go to d_out + dst_off.
 * `ranges` is a host array, read before the call returns.  d_frame, d_out,
 * src_off, len and dst_off may have any byte alignment.  n_ranges == 0 and
 * len == 0 are valid.  Source ranges may overlap or repeat; destinations of
 * non-empty ranges may not overlap.
 *
 * The frame check of fsehip_frame_decompress runs first (header == info, the
 * directory's record lengths end at frame_len): a frame that fails it gets
 * d_result[0] = BAD_FRAME, every range status BAD_FRAME (empty ranges
 * included, d_result[1] = n_ranges), and no byte of d_out is touched.
 * Otherwise the stores are exactly the bytes [d_out + dst_off, d_out +
 * dst_off + len) of each range, minus the portions that come from failed
 * blocks: a block that fails (a bad directory entry or a decoder status, as
 * in fsehip_frame_decompress) loses only its own bytes, in every range that
 * touches it.  d_range_status (n_ranges entries, may be NULL): FSE_OK or the
 * status of the lowest-numbered failed block the range touches.  d_result[0]
 * = frame status, d_result[1] = ranges with a failed block.
 *
 * Work: only the header, the directory (up to the last covered block) and
 * the records of covered blocks are read; blocks no range covers are never
 * unpacked or decoded, so their records may hold anything as long as the
 * directory's lengths still add up.  A host planner lists the covered blocks
 * once each, and one directory pass (a seek kernel) gives their record
 * offsets.  Two routes:
 *   direct  a run of >= 4 whole blocks of one range whose destination start
 *           is 16-byte aligned (the frame's last block counts as whole when
 *           the range ends at n_total) goes through the chunk loop of
 *           fsehip_frame_decompress with the output shifted, in place;
 *   bounce  every other piece: the listed blocks' FSE records are gathered
 *           into slot scratch and decoded, a chunk at a time, into a raw
 *           bounce buffer, and a piece kernel (one workgroup per piece)
 *           copies each piece to its destination; RAW pieces are copied and
 *           RLE pieces filled straight from the record.
 * A covered block is unpacked and decoded once per call, with one
 * exception: a block that a direct run decodes in place for one range and of
 * which another range (or the same source range sent to a second
 * destination) needs a piece is decoded again on the bounce route.
 *
 * Chunks hold at most chunk_blocks blocks (0 = 4096, and few enough that
 * the slots stay within 1 GiB); the chunk scratch is sized by the largest
 * chunk the call runs, not by chunk_blocks.  The workspace entries are listed
 * in the note at fsehip_decompress_blocks.  The lists travel through pinned
 * host staging owned by the workspace (up to 8 buffers of 64 KiB, or of the
 * next power of two that holds the lists; with 8 earlier uploads of the
 * stream still pending the call waits for the oldest, and a call whose lists
 * outgrow every free buffer regrows one, which waits for the device).
 * Asynchronous on `stream`, no host synchronisation except then and when the
 * workspace grows; the call holds the stream's workspace throughout.
 *
 * Before any device use: BAD_ARG (a null info, d_frame, d_result, ranges
 * with n_ranges > 0, or d_out with a non-empty range; an `info` that
 * fsehip_frame_read_header would reject; src_off + len overflowing or past
 * info->n_total; dst_off + len overflowing; overlapping destinations),
 * DST_TOO_SMALL (dst_off + len > out_cap), UNSUPPORTED and NO_DEVICE as
 * fsehip_frame_decompress. */
int fsehip_frame_decompress_ranges(const fsehip_frame_info* info, uint32_t chunk_blocks, const uint8_t* d_frame,
                                   uint64_t frame_len, const fsehip_frame_range* ranges, uint32_t n_ranges,
                                   uint8_t* d_out, uint64_t out_cap, int32_t* d_range_status, int32_t* d_result,
                                   fsehip_stream_t stream);
/* The one-range call with dst_off = 0 and no range status: d_result[1] != 0
 * tells that a block of the range failed. */
int fsehip_frame_decompress_range(const fsehip_frame_info* info, uint32_t chunk_blocks, const uint8_t* d_frame,
                                  uint64_t frame_len, uint64_t src_off, uint64_t len, uint8_t* d_out, uint64_t out_cap,
                                  int32_t* d_result, fsehip_stream_t stream);

/* ------------------------------------------------------------------------
 * (2d) The plane frame: a byte-plane split for 2-, 4- and 8-byte elements
 *
 * bf16 / fp16 / fp32 tensors and int32 / int64 indices interleave one
 * compressible byte per element (sign and exponent, the high bytes of small
 * integers) with one to seven nearly random ones; one order-0 table per block
 * averages them.  The plane frame puts byte k of every element into plane k
 * and codes the planes with one unchanged frame of section 2b, whose encoder
 * rule does the rest: exponent planes become FSE blocks, mantissa planes RAW
 * blocks, the zero high planes of small integers RLE blocks.  This library's
 * own container, version 1; integers little-endian, any byte address:
 *
 *    0  u8[4] magic "FSEP"
 *    4  u8    version = 1
 *    5  u8    elem_bytes w: 2, 4 or 8
 *    6  u16   reserved = 0
 *    8  u64   n_elems
 *   16  one frame (section 2b) of the plane image, to the end of the buffer
 *
 * Plane image: with stride = roundup(n_elems, 16),
 * image[k * stride + i] = raw[i * w + k] for k < w, i < n_elems (byte 0 is the
 * element's lowest-addressed byte); the stride - n_elems pad bytes of each
 * plane are zero, so plane frames are deterministic.  The inner frame's
 * n_total must equal w * stride.  n_elems = 0 is valid: 16 + 32 bytes.  Planes
 * share the inner frame, so at most w - 1 blocks straddle two planes.  The
 * container stores the element width, not the dtype or the shape.
 * ------------------------------------------------------------------------ */

typedef struct {
    uint32_t version, elem_bytes, reserved, pad_; /* pad_ is not stored */
    uint64_t n_elems;
    uint64_t stride; /* roundup(n_elems, 16): derived, not stored */
} fsehip_planes_info;

/* 16 + fsehip_frame_bound(w * stride, block_size): a capacity no plane frame
 * of n_elems elements exceeds.  0 for elem_bytes outside {2, 4, 8} or when a
 * size overflows 64 bits. */
uint64_t fsehip_planes_bound(uint64_t n_elems, uint32_t elem_bytes, uint32_t block_size);
/* w * stride, the plane image's bytes: the scratch of fsehip_planes_compress /
 * fsehip_planes_decompress and the destination of fsehip_planes_split.  0 for
 * a bad elem_bytes or on overflow (and for n_elems = 0). */
uint64_t fsehip_planes_scratch_bytes(uint64_t n_elems, uint32_t elem_bytes);
/* Parse and validate the first 48 bytes of a plane frame (host pointer; len =
 * bytes available): its own 16 into `out`, the inner frame's header into
 * `inner`.  FSE_ERR_BAD_FRAME for len < 48, bad magic or version, elem_bytes
 * outside {2, 4, 8}, a nonzero reserved field, w * stride overflowing, an
 * inner header fsehip_frame_read_header rejects, or an inner n_total other
 * than w * stride. */
int fsehip_planes_read_header(const uint8_t* hdr, size_t len, fsehip_planes_info* out, fsehip_frame_info* inner);
/* The 16 header bytes of `info` (stride and pad_ are not stored); BAD_ARG when
 * the fields would not pass fsehip_planes_read_header. */
int fsehip_planes_write_header(const fsehip_planes_info* info, uint8_t hdr[16]);

/* The bare transforms, asynchronous on `stream`.
 *  fsehip_planes_split: n_elems elements of elem_bytes at d_src -> the plane
 *    image at d_dst (fsehip_planes_scratch_bytes, 16-byte aligned), pads
 *    zeroed.  d_src need only be aligned to elem_bytes; reads of it go up to
 *    roundup(n_elems * elem_bytes, 4) at most.
 *  fsehip_planes_merge: the plane image at d_src (16-byte aligned) -> exactly
 *    the n_elems * elem_bytes bytes at d_dst (16-byte aligned).
 * BAD_ARG (a null or misaligned pointer with n_elems > 0), UNSUPPORTED
 * (elem_bytes outside {2, 4, 8}; w * stride overflowing) and NO_DEVICE before
 * any device use.  n_elems == 0 returns FSE_OK and does nothing. */
int fsehip_planes_split(uint32_t elem_bytes, const void* d_src, uint64_t n_elems, uint8_t* d_dst,
                        fsehip_stream_t stream);
int fsehip_planes_merge(uint32_t elem_bytes, const uint8_t* d_src, uint64_t n_elems, void* d_dst,
                        fsehip_stream_t stream);

/* Compress n_elems elements of elem_bytes at d_src (aligned to elem_bytes)
 * into one plane frame at d_out (any alignment; out_cap >= fsehip_planes_bound,
 * else DST_TOO_SMALL): split into d_scratch (16-byte aligned, scratch_cap >=
 * fsehip_planes_scratch_bytes, else DST_TOO_SMALL), fsehip_frame_compress of
 * the image to d_out + 16, then the header and *d_out_len = 16 + the frame's
 * length, written on the device in stream order.  d_result as in
 * fsehip_frame_compress.  Only the first *d_out_len bytes of d_out are
 * written.  The library allocates nothing for the planes (the frame call's
 * workspace apart).  Call-level statuses as fsehip_frame_compress, with
 * UNSUPPORTED also for elem_bytes outside {2, 4, 8}; all before any device
 * use. */
int fsehip_planes_compress(const fsehip_frame_params* p, uint32_t elem_bytes, const void* d_src, uint64_t n_elems,
                           uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
                           uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream);

/* Decompress the plane frame of in_len bytes at d_in (any alignment) whose
 * first 48 bytes fsehip_planes_read_header parsed into `info` and `inner`:
 * fsehip_frame_decompress of d_in + 16 into d_scratch (as above), then the
 * merge into d_out (16-byte aligned; out_cap >= n_elems * elem_bytes, else
 * DST_TOO_SMALL).  d_block_status (inner->n_blocks entries, may be NULL) and
 * d_result are the frame call's.  The 16 header bytes on the device must equal
 * `info`, and the frame check of fsehip_frame_decompress must pass: otherwise
 * d_result[0] = BAD_FRAME, every block status BAD_FRAME, and no byte of d_out
 * is touched.  A failed inner block leaves unspecified bytes in the elements
 * that have a byte in it, and nowhere else.  BAD_ARG also for in_len < 48 and
 * for an `info` / `inner` pair fsehip_planes_read_header would reject. */
int fsehip_planes_decompress(const fsehip_planes_info* info, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                             const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap,
                             void* d_out, uint64_t out_cap, int32_t* d_block_status, int32_t* d_result,
                             fsehip_stream_t stream);

/* One element range of a plane frame and where it goes (element units). */
typedef struct {
    uint64_t elem_off;     /* first element of the range */
    uint64_t n_elems;      /* elements; 0 is valid */
    uint64_t dst_elem_off; /* the range goes to d_out + dst_elem_off * elem_bytes */
} fsehip_planes_range;

/* The scratch fsehip_planes_decompress_ranges needs for a range list (host
 * array): each range's w plane pieces, 16-byte aligned per range, then one
 * int32 per plane piece.  0 for a bad elem_bytes or on overflow. */
uint64_t fsehip_planes_ranges_scratch_bytes(uint32_t elem_bytes, const fsehip_planes_range* ranges,
                                            uint32_t n_ranges);

/* Decode element ranges of a plane frame without decoding the rest: range r
 * becomes the w byte ranges k * stride + elem_off of the inner frame, all in
 * one fsehip_frame_decompress_ranges call into d_scratch (16-byte aligned),
 * so only the covered blocks are decoded; a pieces kernel then interleaves
 * the plane pieces into d_out.  d_out may have any byte alignment.  Stores:
 * exactly the n_elems * elem_bytes bytes of each range.  d_range_status
 * (n_ranges entries, may be NULL): the status of the range's first failing
 * plane range; d_result[0] = frame status, d_result[1] = element ranges with
 * a failure.  On BAD_FRAME (the header on the device differs from `info`, or
 * the inner frame check fails) every range status is BAD_FRAME and no byte of
 * d_out is touched.  `ranges` is a host array, read before the call returns;
 * the per-range parameters reach the device as kernel arguments, in stream
 * order and with no host synchronisation of their own.
 *
 * Before any device use, in element units as fsehip_frame_decompress_ranges
 * in bytes: BAD_ARG (a null pointer; in_len < 48; a bad info / inner pair;
 * elem_off + n_elems overflowing or past info->n_elems; dst_elem_off +
 * n_elems overflowing; overlapping destinations of non-empty ranges; a
 * misaligned d_scratch), DST_TOO_SMALL ((dst_elem_off + n_elems) * elem_bytes
 * > out_cap, or scratch_cap below fsehip_planes_ranges_scratch_bytes),
 * UNSUPPORTED (more than 2^32 - 1 plane ranges), NO_DEVICE.  n_ranges == 0
 * and empty ranges are valid. */
int fsehip_planes_decompress_ranges(const fsehip_planes_info* info, const fsehip_frame_info* inner,
                                    uint32_t chunk_blocks, const uint8_t* d_in, uint64_t in_len,
                                    const fsehip_planes_range* ranges, uint32_t n_ranges, uint8_t* d_scratch,
                                    uint64_t scratch_cap, void* d_out, uint64_t out_cap, int32_t* d_range_status,
                                    int32_t* d_result, fsehip_stream_t stream);

/* ------------------------------------------------------------------------
 * (2e) The delta frame: element delta with restarts for integer tensors
 *
 * Index tensors that grow -- sorted ids, CSR and embedding-bag offsets,
 * timestamps, sampled signals -- keep most of their bytes live under the
 * plane split of section 2d, because the values grow; their differences are
 * small.  The delta frame codes the zigzag differences of neighbouring
 * elements, split into byte planes, with one unchanged frame of section 2b.
 * This library's own container, version 1; integers little-endian, any byte
 * address:
 *
 *    0  u8[4] magic "FSED"
 *    4  u8    version = 1
 *    5  u8    elem_bytes w: 1, 2, 4 or 8
 *    6  u16   reserved = 0
 *    8  u64   n_elems
 *   16  one frame (section 2b) of the delta image, to the end of the buffer
 *
 * Delta image: the elements are read as unsigned little-endian integers x_i
 * of w bytes, whatever the dtype, and all arithmetic is mod 2^(8 w).
 *   d_i = x_i                 when i % FSEHIP_DELTA_RESTART == 0,
 *         x_i - x_(i-1)       otherwise;
 *   z_i = (d_i << 1) ^ (0 - (d_i >> (8 w - 1)))            (zigzag);
 *   image[k * stride + i] = byte k of z_i, k < w, i < n_elems,
 * with stride = roundup(n_elems, 16) and the stride - n_elems pad bytes of
 * each plane zero: for w = 2, 4, 8 the plane image (section 2d) of z, for
 * w = 1 z itself, padded.  The inner frame's n_total must equal w * stride.
 * Decode: d_i = (z_i >> 1) ^ (0 - (z_i & 1)), and x_i = the sum of d from the
 * first element of i's restart group through i.  The restart interval is a
 * constant of version 1, not a header field: an element range needs only its
 * own restart groups (4096 bytes per plane each), so byte-range decode of the
 * inner frame keeps working, and no sum ever crosses a group.  n_elems = 0 is
 * valid: 16 + 32 bytes.  The container stores the element width, not the
 * dtype or the shape.  The filter is for integers; floats gain nothing
 * (DESIGN.md section 5 "Delta").
 * ------------------------------------------------------------------------ */

#define FSEHIP_DELTA_RESTART 4096u /* elements between restarts, version 1 */

typedef fsehip_planes_info fsehip_delta_info; /* the same fields (section 2d) */

/* 16 + fsehip_frame_bound(w * stride, block_size): a capacity no delta frame
 * of n_elems elements exceeds.  0 for elem_bytes outside {1, 2, 4, 8} or when
 * a size overflows 64 bits. */
uint64_t fsehip_delta_bound(uint64_t n_elems, uint32_t elem_bytes, uint32_t block_size);
/* w * stride, the delta image's bytes: the scratch of fsehip_delta_compress /
 * fsehip_delta_decompress and the destination of fsehip_delta_encode.  0 for
 * a bad elem_bytes or on overflow (and for n_elems = 0). */
uint64_t fsehip_delta_scratch_bytes(uint64_t n_elems, uint32_t elem_bytes);
/* Parse and validate the first 48 bytes of a delta frame (host pointer; len =
 * bytes available), as fsehip_planes_read_header: BAD_FRAME for len < 48, bad
 * magic or version, elem_bytes outside {1, 2, 4, 8}, a nonzero reserved
 * field, w * stride overflowing, an inner header fsehip_frame_read_header
 * rejects, or an inner n_total other than w * stride.  Outputs are zeroed on
 * every reject. */
int fsehip_delta_read_header(const uint8_t* hdr, size_t len, fsehip_delta_info* out, fsehip_frame_info* inner);
/* The 16 header bytes of `info` (stride and pad_ are not stored); BAD_ARG when
 * the fields would not pass fsehip_delta_read_header. */
int fsehip_delta_write_header(const fsehip_delta_info* info, uint8_t hdr[16]);

/* The bare transforms, asynchronous on `stream`.
 *  fsehip_delta_encode: n_elems elements of elem_bytes at d_src -> the delta
 *    image at d_dst (fsehip_delta_scratch_bytes, 16-byte aligned), pads
 *    zeroed.  d_src need only be aligned to elem_bytes; reads of it go up to
 *    roundup(n_elems * elem_bytes, 4) at most.
 *  fsehip_delta_decode: the delta image at d_src (16-byte aligned) -> exactly
 *    the n_elems * elem_bytes bytes at d_dst (16-byte aligned).
 * BAD_ARG (a null or misaligned pointer with n_elems > 0), UNSUPPORTED
 * (elem_bytes outside {1, 2, 4, 8}; w * stride overflowing) and NO_DEVICE
 * before any device use.  n_elems == 0 returns FSE_OK and does nothing. */
int fsehip_delta_encode(uint32_t elem_bytes, const void* d_src, uint64_t n_elems, uint8_t* d_dst,
                        fsehip_stream_t stream);
int fsehip_delta_decode(uint32_t elem_bytes, const uint8_t* d_src, uint64_t n_elems, void* d_dst,
                        fsehip_stream_t stream);

/* fsehip_planes_compress with the delta image in place of the plane image:
 * the same arguments, alignment rules (d_src to elem_bytes, d_scratch to 16,
 * d_out any), capacities (fsehip_delta_scratch_bytes, fsehip_delta_bound) and
 * statuses, UNSUPPORTED for elem_bytes outside {1, 2, 4, 8}; nothing
 * allocated for the transform, no host synchronisation. */
int fsehip_delta_compress(const fsehip_frame_params* p, uint32_t elem_bytes, const void* d_src, uint64_t n_elems,
                          uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
                          uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream);

/* fsehip_planes_decompress for a delta frame whose first 48 bytes
 * fsehip_delta_read_header parsed into `info` and `inner`: the same
 * arguments, rules and statuses (d_out 16-byte aligned); on BAD_FRAME every
 * block status is BAD_FRAME and no byte of d_out is touched.  A failed inner
 * block costs the elements from the first one with a byte in it to the end of
 * their restart groups (their sums run through it); every other element is
 * exact. */
int fsehip_delta_decompress(const fsehip_delta_info* info, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                            const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap,
                            void* d_out, uint64_t out_cap, int32_t* d_block_status, int32_t* d_result,
                            fsehip_stream_t stream);

/* The scratch fsehip_delta_decompress_ranges needs for a range list (host
 * array).  A range is decoded from e0 = elem_off rounded down to a multiple
 * of FSEHIP_DELTA_RESTART: per range w plane pieces of
 * roundup(elem_off + n_elems - e0, 16) bytes, then one int32 per plane piece,
 * rounded up to 16.  0 for a bad elem_bytes or on overflow. */
uint64_t fsehip_delta_ranges_scratch_bytes(uint32_t elem_bytes, const fsehip_planes_range* ranges,
                                           uint32_t n_ranges);

/* fsehip_planes_decompress_ranges for a delta frame: each non-empty range
 * becomes the w byte ranges k * stride + e0 .. k * stride + elem_off + n_elems
 * of the inner frame, one fsehip_frame_decompress_ranges call into d_scratch
 * decodes only the blocks they cover, and a pieces kernel sums each restart
 * group and stores exactly the n_elems * elem_bytes bytes of each range at
 * d_out + dst_elem_off * elem_bytes (any byte alignment).  The range rules,
 * statuses (d_range_status, d_result) and argument checks are those of
 * fsehip_planes_decompress_ranges, with fsehip_delta_ranges_scratch_bytes for
 * the scratch.  A range's status covers the blocks from e0 on. */
int fsehip_delta_decompress_ranges(const fsehip_delta_info* info, const fsehip_frame_info* inner,
                                   uint32_t chunk_blocks, const uint8_t* d_in, uint64_t in_len,
                                   const fsehip_planes_range* ranges, uint32_t n_ranges, uint8_t* d_scratch,
                                   uint64_t scratch_cap, void* d_out, uint64_t out_cap, int32_t* d_range_status,
                                   int32_t* d_result, fsehip_stream_t stream);

/* ------------------------------------------------------------------------
 * (2f) The check record and sealed buffers: per-block CRC-32 of the content
 *
 * The containers of sections 2b, 2d and 2e tell a reader what the format can
 * see (a bad header, a missing marker, a checkpoint that disagrees); a RAW
 * record is copied unchecked, and an FSE payload with a flipped bit very
 * often still decodes with FSE_OK.  The check record holds CRC-32s of the
 * CONTENT -- what the user handed in and gets back; for a plane or delta
 * frame the tensor's n_elems * w bytes, not the image -- one per check block,
 * and travels in front of an unchanged container.  Version 1; integers
 * little-endian, no padding, any byte address:
 *
 *   header, 32 bytes
 *      0  u8[4] magic "FSEK"
 *      4  u8    version = 1
 *      5  u8    algorithm = 1   (FSEHIP_CHECK_CRC32)
 *      6  u8    check_log       log2 of check_block, 8..16 (256 B .. 64 KiB)
 *      7  u8    0
 *      8  u64   n_content       bytes of content
 *     16  u32   n_cb            = ceil(n_content / check_block); 0 when empty
 *     20  u32   content_crc     CRC-32 of the whole content; 0 when empty
 *     24  u32   reserved = 0
 *     28  u32   header_crc      CRC-32 of bytes 0..27
 *   table, n_cb x u32: CRC-32 of content[b * check_block,
 *                                        min((b + 1) * check_block, n_content))
 *
 * The CRC is zlib's: reflected polynomial 0xEDB88320, initial value and final
 * XOR 0xFFFFFFFF, so content_crc = zlib.crc32(content) and any reader can
 * check it.  CRCs combine exactly, crc(A || B) = crc(A) * x^(8 |B|) mod P xor
 * crc(B), so content_crc is the combine of the table and costs no second
 * pass, damage is localised to one check block, and a range read can verify
 * the blocks it covers.  A small check_log buys finer coverage -- of damage
 * and of ranges -- at 4 bytes per check block: 4 / 2^check_log of the content
 * (0.006 % at 16, 1.6 % at 8).
 *
 * A SEALED BUFFER is a check record followed directly by exactly one
 * container of section 2b, 2d, 2e or 2h; the container's magic says which.  The
 * container's content length (n_total; n_elems * w) must equal n_content and
 * the buffer ends with the container: anything else is BAD_FRAME.  The
 * record's size is known before anything runs, so the container is
 * compressed straight to its final place, fsehip_check_bytes into the buffer.
 * Nothing in sections 2b, 2d or 2e changes.
 * ------------------------------------------------------------------------ */

#define FSEHIP_CHECK_CRC32 1u
#define FSEHIP_SEALED_FRAME 0u  /* `kind` of fsehip_sealed_read_header */
#define FSEHIP_SEALED_PLANES 1u
#define FSEHIP_SEALED_DELTA 2u
#define FSEHIP_SEALED_DIFF 3u   /* a diff frame (section 2h): decoding needs the base */

typedef struct {
    uint32_t version, algorithm, check_log, reserved; /* reserved: byte 7 | the word at 24 */
    uint64_t n_content;
    uint32_t n_cb, content_crc;
    uint32_t header_crc, pad_; /* pad_ is not stored */
} fsehip_check_info;

/* zlib's crc32(crc, buf, len) and crc32_combine(crc1, crc2, len2), host
 * memory, no device: fsehip_crc32(0, NULL, 0) = 0 is the initial value,
 * fsehip_crc32(fsehip_crc32(0, a, n), b, m) the CRC of a || b, and
 * fsehip_crc32_combine(crc(a), crc(b), m) the same.  Part of the format, as
 * the header readers are. */
uint32_t fsehip_crc32(uint32_t crc, const uint8_t* buf, size_t n);
uint32_t fsehip_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);

/* 32 + 4 * n_cb: the record's size for n_content bytes (check_log 0 = 16).
 * 0 for a check_log outside 8..16 or when n_cb does not fit 32 bits. */
uint64_t fsehip_check_bytes(uint64_t n_content, uint32_t check_log);
/* Parse and validate the first 32 bytes of a check record (host pointer; len
 * = bytes available).  FSE_ERR_BAD_FRAME for len < 32, a bad magic, version,
 * algorithm or check_log, a nonzero byte 7 or reserved word, an n_cb other
 * than ceil(n_content / check_block), a nonzero content_crc with n_content =
 * 0, or a wrong header_crc.  `out` is zeroed on every reject. */
int fsehip_check_read_header(const uint8_t* hdr, size_t len, fsehip_check_info* out);
/* The 32 header bytes of `info`, the host's way to make a record: header_crc
 * is computed here (info->header_crc is not read).  BAD_ARG when the other
 * fields would not pass fsehip_check_read_header. */
int fsehip_check_write_header(const fsehip_check_info* info, uint8_t hdr[32]);
/* The head of a sealed buffer (host pointer; len = bytes available, at least
 * the record and the first 32 bytes of a frame or 48 of a plane, delta or
 * diff frame): the record's header into `info`, the container's kind from its
 * magic, and *inner_off = 32 + 4 * n_cb, where the container starts.
 * BAD_FRAME for a record fsehip_check_read_header rejects, a head too short,
 * another magic, or a container whose content length is not n_content.  The
 * container's header is then read with its own reader at buf + *inner_off. */
int fsehip_sealed_read_header(const uint8_t* buf, size_t len, fsehip_check_info* info, uint32_t* kind,
                              uint64_t* inner_off);

/* Write the whole record of n_content bytes at d_content to d_record
 * (fsehip_check_bytes(n_content, check_log) bytes; check_log 0 = 16): one CRC
 * kernel over the content, then a finish kernel that combines the table into
 * content_crc (a tree over runs of entries, not a serial walk) and writes the
 * header.  d_content and d_record may have any byte alignment; the content is
 * read in whole aligned 16-byte words that hold at least one of its bytes.
 * n_content == 0 writes a 32-byte record.  Asynchronous on `stream`, no host
 * synchronisation, no workspace.  Before any device use: BAD_ARG (a null
 * d_record, a null d_content with n_content > 0), UNSUPPORTED (a check_log
 * outside 8..16, n_cb above 2^32 - 1), NO_DEVICE. */
int fsehip_check_build(uint32_t check_log, const uint8_t* d_content, uint64_t n_content, uint8_t* d_record,
                       fsehip_stream_t stream);

/* Compare the record at d_record, whose header fsehip_check_read_header
 * parsed into `info`, with the n_content bytes at d_content (n_content must
 * equal info->n_content: BAD_ARG).  The 32 header bytes on the device must
 * equal `info`: otherwise d_result[0] = BAD_FRAME, every check status
 * BAD_FRAME and d_result[1] = n_cb.  Otherwise d_check_status[b] (n_cb
 * entries, required when n_cb > 0; it also holds the computed CRCs between
 * the kernels) = FSE_OK or FSE_ERR_CHECKSUM, d_result[1] = failed check
 * blocks, and d_result[0] = FSE_ERR_CHECKSUM when the combine of the COMPUTED
 * block CRCs differs from content_crc, else FSE_OK.  Nothing is stored into
 * the content or the record.  Alignment, reads and call-level statuses as
 * fsehip_check_build (BAD_ARG also for a null or invalid `info`, a null
 * d_result). */
int fsehip_check_verify(const fsehip_check_info* info, const uint8_t* d_record, const uint8_t* d_content,
                        uint64_t n_content, int32_t* d_check_status, int32_t* d_result, fsehip_stream_t stream);

/* How many bytes of a range request fsehip_check_verify_ranges covers: the
 * check blocks that lie wholly inside a range, summed over the ranges.
 * BAD_ARG for an invalid info, or src_off + len overflowing or past
 * n_content. */
int fsehip_check_ranges_verified_bytes(const fsehip_check_info* info, const fsehip_frame_range* ranges,
                                       uint32_t n_ranges, uint64_t* bytes);

/* Verify decoded ranges: `ranges` are the triples of
 * fsehip_frame_decompress_ranges in content bytes, range r's bytes lying at
 * d_out + dst_off (any alignment).  For each range every check block that
 * lies wholly inside [src_off, src_off + len) is verified; the content's last
 * block counts as whole when the range ends at n_content.  Partial blocks at
 * a range's edges are NOT verified -- they cannot be without decoding more
 * than was asked for; a smaller check_log leaves less uncovered.
 * d_range_status[r] (n_ranges entries, required when n_ranges > 0) = FSE_OK
 * or FSE_ERR_CHECKSUM; d_result[0] = FSE_OK, d_result[1] = ranges with a
 * failed check block.  A header on the device that differs from `info`:
 * d_result[0] = BAD_FRAME, every range status BAD_FRAME, d_result[1] =
 * n_ranges.  The ranges reach the device as kernel arguments, 32 per launch:
 * no staging, no host synchronisation.  Before any device use: BAD_ARG (a
 * null pointer, an invalid info, a range overflowing or past n_content,
 * overlapping destinations of non-empty ranges), DST_TOO_SMALL (dst_off + len
 * > out_cap), NO_DEVICE. */
int fsehip_check_verify_ranges(const fsehip_check_info* info, const uint8_t* d_record,
                               const fsehip_frame_range* ranges, uint32_t n_ranges, const uint8_t* d_out,
                               uint64_t out_cap, int32_t* d_range_status, int32_t* d_result, fsehip_stream_t stream);

/* ------------------------------------------------------------------------
 * (2g) Size estimates: which of the frame, the plane frame and the delta
 *      frame is smallest for a tensor, without compressing it
 *
 * A wrong container costs up to 3.4x in size; finding
 * the right one by compressing three times costs three encodes and three
 * output buffers.  The estimate predicts each container's length from the
 * 256-bin byte counts of every block of its image -- the raw bytes, the plane
 * image (section 2d) or the delta image (section 2e), the latter two counted
 * from the source without writing the image -- and from the encoder's own
 * normalisation and header writer.  No format changes: the estimate only
 * chooses which existing call to make.
 *
 * The estimate is integer arithmetic throughout, so every implementation
 * gives the same numbers (tests/estimate_ref.py restates it):
 *
 *   log2q8(c), 1 <= c <= 32768:  hb = floor(log2 c); x = c << (31 - hb) as a
 *     u64; y = hb; eight times { x = (x * x) >> 31; y <<= 1; if (x >> 32)
 *     { x >>= 1; y |= 1; } }; the result y is within 1.01 of 256 * log2 c and
 *     exact at powers of two.
 *   cost8(c, L) = 256 * L - log2q8(max(c, 1)): 256 x the bits of a symbol
 *     whose normalised count is c at table log L; a count of -1 costs L bits.
 *
 *   One block, from its byte counts cnt[256], its raw_len and the frame
 *   parameters nstates, ckpt_interval, table_log (0 = the crate's optimal
 *   log) and max_table_log:
 *     RLE, 1 byte, iff cnt[0] == raw_len and raw_len > 0.
 *     RAW, raw_len bytes, when the encoder status the histogram alone
 *       determines is not FSE_OK: TOO_SHORT (raw_len < 2), CURSED (a
 *       histogram Histogram::normalize refuses), or a table log above the
 *       kernel class of max_table_log (the encoder's UNSUPPORTED).
 *     Otherwise, with norm[] and L from the encoder's normalisation and hdr
 *       the exact byte length of NormHistogram::write:
 *         Q    = sum over s of cnt[s] * cost8(norm[s], L)           (u64)
 *         bits = ((Q + 255) >> 8) + nstates * L + 1
 *         comp = hdr + ceil(bits / 8)
 *         rec  = comp + 8 * fsehip_sidecar_per_block_ns(raw_len, ckpt_interval, nstates)
 *       and the block is FSE of rec bytes iff rec < raw_len, else RAW.
 *   A frame: 32 + 4 * n_blocks + the sum of its blocks' bytes.  A plane or
 *   delta frame: 16 + the frame estimate of its image.
 *   The choice: the smallest estimate; ties go to the frame, then the plane
 *   frame, then the delta frame.
 *
 * ENCODER_INIT (a block whose coder cannot start, stored RAW) depends on the
 * order of the bytes, which a histogram does not hold: it is not predicted,
 * and such a block is estimated as FSE.  The model's error against real
 * containers is in DESIGN.md section 5 "Estimate" (under 1 % of the length on
 * the tensors measured there); it is an estimate, never a bound: capacities
 * stay fsehip_frame_bound and its kin.
 * ------------------------------------------------------------------------ */

#define FSEHIP_KIND_FRAME 0u  /* section 2b, magic "FSEF" */
#define FSEHIP_KIND_PLANES 1u /* section 2d, magic "FSEP" */
#define FSEHIP_KIND_DELTA 2u  /* section 2e, magic "FSED" */
#define FSEHIP_KIND_SEALED 3u /* section 2f, magic "FSEK": fsehip_container_kind only */
#define FSEHIP_KIND_DIFF 4u   /* section 2h, magic "FSEB": fsehip_container_kind and the calls of section 2i */
#define FSEHIP_EST_NONE UINT64_MAX /* an estimate that was not asked for or does not exist */
#define FSEHIP_EST_RAW 0u /* block types, the frame directory's */
#define FSEHIP_EST_RLE 1u
#define FSEHIP_EST_FSE 2u

typedef struct {
    uint32_t type;      /* FSEHIP_EST_RAW / _RLE / _FSE */
    uint32_t rec;       /* the record's bytes, checkpoints included */
    uint32_t bits;      /* payload bits of an FSE block, else 0 */
    uint32_t table_log; /* of an FSE block, else 0 */
} fsehip_block_estimate;

/* Host functions, no device.
 *  fsehip_log2q8: as defined above; 0 for c outside 1..32768.
 *  fsehip_estimate_choose: the kind of the smallest entry of est[3] (indexed
 *    by kind) under the tie rule; entries of FSEHIP_EST_NONE do not take
 *    part, and -1 when all three are (or est is null).
 *  fsehip_estimate_block_host: the block rule applied to a caller's table:
 *    counts[256] and raw_len as above; norm[256], norm_log and hdr_bytes the
 *    normalised counts, their table log and the header length the caller got
 *    from the normalisation (norm null: the statistics refused the block);
 *    nstates, ckpt_interval and max_table_log from p.  BAD_ARG for a null
 *    counts, p or out, nstates above 2, norm_log outside 5..15 or a nonzero
 *    count whose norm entry is 0 or above 2^norm_log.
 *  fsehip_container_kind: the FSEHIP_KIND_* value of a buffer's magic (host
 *    pointer, len = bytes available; a sealed buffer reports
 *    FSEHIP_KIND_SEALED, its container's kind is fsehip_sealed_read_header's;
 *    a diff frame of section 2h FSEHIP_KIND_DIFF, which the estimate calls of
 *    section 2i take and those of this section refuse; a pack frame of
 *    section 2j FSEHIP_KIND_PACK, a versioned pack of section 2k
 *    FSEHIP_KIND_VPACK and a sealed pack of section 2l FSEHIP_KIND_SPACK),
 *    FSE_ERR_BAD_FRAME for len < 4 or any other magic, BAD_ARG for a null buf
 *    with len > 0.  Only the magic is read; the headers have their readers. */
uint32_t fsehip_log2q8(uint32_t c);
int fsehip_estimate_choose(const uint64_t est[3]);
int fsehip_estimate_block_host(const uint32_t counts[256], uint32_t raw_len, const int32_t norm[256],
                               uint32_t norm_log, uint32_t hdr_bytes, const fsehip_frame_params* p,
                               fsehip_block_estimate* out);
int fsehip_container_kind(const uint8_t* buf, size_t len);

/* The bytes a kind's inner frame codes for n_elems elements of elem_bytes:
 * n_elems * elem_bytes (FRAME), the plane image's (PLANES) or the delta
 * image's (DELTA).  0 for a kind above 2, elem_bytes outside {1, 2, 4, 8},
 * PLANES at elem_bytes 1, on overflow, and for n_elems = 0. */
uint64_t fsehip_estimate_image_bytes(uint32_t kind, uint64_t n_elems, uint32_t elem_bytes);

/* Per-block 256-bin counts of a kind's image: d_counts[b * 256 + s] = how
 * often byte s occurs in image bytes [b * block_size, (b + 1) * block_size),
 * for the ceil(fsehip_estimate_image_bytes / block_size) blocks (block_size
 * 0 = 65536).  FRAME is fsehip_histogram_blocks over the raw bytes; PLANES
 * (elem_bytes 2, 4, 8) and DELTA (1, 2, 4, 8) read the source once and write
 * no image: the zero pads up to the stride are counted, and blocks that
 * straddle two planes hold bytes of both, exactly as the image's blocks do.
 * d_src aligned to elem_bytes (reads go up to roundup(n_elems * elem_bytes,
 * 4) at most), d_counts to 4.  Asynchronous on `stream`, no host
 * synchronisation, no workspace.  Before any device use: BAD_ARG (kind above
 * 2, a null or misaligned pointer with n_elems > 0, more than one block of a
 * size that is no multiple of 16, more than 2^32 - 1 blocks), UNSUPPORTED
 * (elem_bytes outside {1, 2, 4, 8}, PLANES at elem_bytes 1, a size
 * overflowing), NO_DEVICE.  n_elems == 0 returns FSE_OK and does nothing. */
int fsehip_image_histogram(uint32_t kind, uint32_t elem_bytes, const void* d_src, uint64_t n_elems,
                           uint32_t block_size, uint32_t* d_counts, fsehip_stream_t stream);

/* The block rule on the device, one wave per block, with the encoder's own
 * optimal_log2 / normalize / header writer: d_counts as
 * fsehip_image_histogram gives them (or a caller's, 256 per block, each
 * block's summing to its raw length) for an image of n_image_bytes in blocks
 * of p->block_size.  Per block b, each output optional (null: not written):
 * d_type[b] (u8, FSEHIP_EST_*), d_rec[b], d_bits[b] and d_log[b] (u8) as in
 * fsehip_block_estimate.  *d_total (required) = 32 + 4 * n_blocks + the sum
 * of rec: the frame estimate.  p's table_log, ckpt_interval, max_table_log
 * and nstates mean what they mean to fsehip_frame_compress; chunk_blocks is
 * not used.  Asynchronous on `stream`, no host synchronisation, no workspace.
 * Before any device use: BAD_ARG (a null p, d_total, or d_counts with
 * n_image_bytes > 0; d_counts, d_rec, d_bits not 4-byte or d_total not 8-byte
 * aligned; nstates above 2; a checkpoint interval fsehip_frame_compress
 * refuses; the block rules of fsehip_frame_compress), UNSUPPORTED (a block
 * size above 2^28), NO_DEVICE. */
int fsehip_estimate_blocks(const fsehip_frame_params* p, const uint32_t* d_counts, uint64_t n_image_bytes,
                           uint8_t* d_type, uint32_t* d_rec, uint32_t* d_bits, uint8_t* d_log, uint64_t* d_total,
                           fsehip_stream_t stream);

/* The scratch of fsehip_estimate: the counts of the largest image among the
 * kinds of kind_mask (bit k = kind k) that take elem_bytes, 1024 bytes per
 * block; the kinds run one after the other on it.  0 for a kind_mask of 0 or
 * above 7, elem_bytes outside {1, 2, 4, 8}, on overflow, and when nothing is
 * needed (n_elems = 0). */
uint64_t fsehip_estimate_scratch_bytes(uint64_t n_elems, uint32_t elem_bytes, uint32_t kind_mask,
                                       uint32_t block_size);

/* The estimated length of each container of kind_mask for the n_elems
 * elements of elem_bytes at d_src, under the frame parameters p: d_est[k]
 * (device, three u64) = the estimate of kind k, or FSEHIP_EST_NONE when bit k
 * of kind_mask is clear or the kind does not take the width (PLANES at
 * elem_bytes 1).  Per kind: the counts zeroed, fsehip_image_histogram,
 * fsehip_estimate_blocks, all on `stream` with no host synchronisation; the
 * caller reads d_est when the stream gets there and calls
 * fsehip_estimate_choose.  d_scratch: fsehip_estimate_scratch_bytes, 16-byte
 * aligned; nothing is allocated and no workspace is held.  n_elems = 0 gives
 * the empty containers' lengths (32, 48, 48).  Before any device use: BAD_ARG
 * (a null p or d_est, kind_mask 0 or above 7, a null d_src or d_scratch with
 * n_elems > 0, d_src not aligned to elem_bytes, d_scratch to 16 or d_est to
 * 8, and fsehip_estimate_blocks' rules for p on every image), UNSUPPORTED
 * (elem_bytes outside {1, 2, 4, 8}, a size overflowing, a block size above
 * 2^28), DST_TOO_SMALL (scratch_bytes below fsehip_estimate_scratch_bytes),
 * NO_DEVICE. */
int fsehip_estimate(const fsehip_frame_params* p, uint32_t kind_mask, uint32_t elem_bytes, const void* d_src,
                    uint64_t n_elems, uint8_t* d_scratch, uint64_t scratch_bytes, uint64_t* d_est,
                    fsehip_stream_t stream);

/* ------------------------------------------------------------------------
 * (2h) The diff frame: a tensor coded as its difference against a base tensor
 *
 * The tensors moved most often are versions of something the receiver already
 * holds: a checkpoint beside the previous one, weights after an optimiser
 * step, a fine-tune beside its base, a table with a few rows replaced.  The
 * diff frame codes the zigzag differences of the elements' bit patterns
 * against the base tensor's, split into byte planes, with one unchanged frame
 * of section 2b.  This library's own container, version 1; integers
 * little-endian, any byte address:
 *
 *    0  u8[4] magic "FSEB"   ("against a base")
 *    4  u8    version = 1
 *    5  u8    elem_bytes w: 1, 2, 4 or 8
 *    6  u16   reserved = 0
 *    8  u64   n_elems
 *   16  one frame (section 2b) of the diff image, to the end of the buffer
 *
 * Diff image: the elements of the tensor x and of the base b, n_elems each,
 * are read as unsigned little-endian integers of w bytes, whatever the dtype,
 * and all arithmetic is mod 2^(8 w).
 *   d_i = x_i - b_i;
 *   z_i = (d_i << 1) ^ (0 - (d_i >> (8 w - 1)))            (zigzag);
 *   image[k * stride + i] = byte k of z_i, k < w, i < n_elems,
 * with stride = roundup(n_elems, 16) and the stride - n_elems pad bytes of
 * each plane zero: for w = 2, 4, 8 the plane image (section 2d) of z, for
 * w = 1 z itself, padded.  The inner frame's n_total must equal w * stride.
 * Decode: d_i = (z_i >> 1) ^ (0 - (z_i & 1)), x_i = b_i + d_i.  There are no
 * restarts: an element depends on its own base element only, so an element
 * range needs its own bytes of each plane and its own base elements, nothing
 * else.  n_elems = 0 is valid: 16 + 32 bytes.  There is one format: subtract
 * and zigzag, no XOR variant and no mode field (DESIGN.md section 5 "Diff").
 *
 * THE CONTAINER DOES NOT IDENTIFY THE BASE.  Decoding against another base
 * gives other bytes with every status FSE_OK.  The guard is the sealed buffer
 * of section 2f: its CRCs are taken over the content, so a wrong base is
 * reported as CHECKSUM for each check block it changes.  "FSEB" is BAD_FRAME
 * to the readers of sections 2b, 2d and 2e, and their magics are BAD_FRAME to
 * this one.
 *
 * The calls mirror section 2d's call for call, with the base, a device
 * pointer to n_elems elements aligned to elem_bytes, after the source or
 * destination pointer.  Their argument rules are the plane calls', and,
 * before any device use: a null d_base with n_elems > 0, or one not aligned
 * to elem_bytes, is BAD_ARG.  The encode side only reads: d_src == d_base is
 * fine (and codes all zeros).
 *
 * IN-PLACE DECODE: fsehip_diff_decode and fsehip_diff_decompress allow d_out
 * == d_base (d_dst == d_base) and then update the base where it lies; any
 * other overlap of [d_out, d_out + n_elems * w) with [d_base, d_base + n_elems
 * * w) is BAD_ARG.  What an in-place decode leaves behind: on BAD_FRAME the
 * base is untouched; after a failed inner block the elements with a byte in
 * that block are undefined -- exactly as out of place, but now the base's
 * values there are gone too.  A caller who cannot lose the base decodes out
 * of place.  fsehip_diff_decompress_ranges allows no overlap of the
 * destinations' extent with the base at all: BAD_ARG.
 * ------------------------------------------------------------------------ */

typedef fsehip_planes_info fsehip_diff_info; /* the same fields (section 2d) */

/* 16 + fsehip_frame_bound(w * stride, block_size): a capacity no diff frame
 * of n_elems elements exceeds (the inner frame's RAW fallback bounds it
 * whatever the base).  0 for elem_bytes outside {1, 2, 4, 8} or when a size
 * overflows 64 bits. */
uint64_t fsehip_diff_bound(uint64_t n_elems, uint32_t elem_bytes, uint32_t block_size);
/* w * stride, the diff image's bytes: the scratch of fsehip_diff_compress /
 * fsehip_diff_decompress and the destination of fsehip_diff_encode.  0 for a
 * bad elem_bytes or on overflow (and for n_elems = 0). */
uint64_t fsehip_diff_scratch_bytes(uint64_t n_elems, uint32_t elem_bytes);
/* Parse and validate the first 48 bytes of a diff frame (host pointer; len =
 * bytes available), as fsehip_planes_read_header: BAD_FRAME for len < 48, bad
 * magic or version, elem_bytes outside {1, 2, 4, 8}, a nonzero reserved
 * field, w * stride overflowing, an inner header fsehip_frame_read_header
 * rejects, or an inner n_total other than w * stride.  Outputs are zeroed on
 * every reject. */
int fsehip_diff_read_header(const uint8_t* hdr, size_t len, fsehip_diff_info* out, fsehip_frame_info* inner);
/* The 16 header bytes of `info` (stride and pad_ are not stored); BAD_ARG when
 * the fields would not pass fsehip_diff_read_header. */
int fsehip_diff_write_header(const fsehip_diff_info* info, uint8_t hdr[16]);

/* The bare transforms, asynchronous on `stream`.
 *  fsehip_diff_encode: n_elems elements of elem_bytes at d_src against those
 *    at d_base -> the diff image at d_dst (fsehip_diff_scratch_bytes, 16-byte
 *    aligned), pads zeroed.  d_src and d_base need only be aligned to
 *    elem_bytes, each on its own; reads of either go up to roundup(n_elems *
 *    elem_bytes, 4) at most.
 *  fsehip_diff_decode: the diff image at d_src (16-byte aligned) and the base
 *    -> exactly the n_elems * elem_bytes bytes at d_dst (16-byte aligned;
 *    d_base itself or clear of it).  Reads of d_base go up to roundup(n_elems
 *    * elem_bytes, 4) at most.
 * BAD_ARG (a null or misaligned pointer with n_elems > 0; a destination that
 * overlaps the base without being it), UNSUPPORTED (elem_bytes outside {1, 2,
 * 4, 8}; w * stride overflowing) and NO_DEVICE before any device use.
 * n_elems == 0 returns FSE_OK and does nothing. */
int fsehip_diff_encode(uint32_t elem_bytes, const void* d_src, const void* d_base, uint64_t n_elems, uint8_t* d_dst,
                       fsehip_stream_t stream);
int fsehip_diff_decode(uint32_t elem_bytes, const uint8_t* d_src, uint64_t n_elems, void* d_dst, const void* d_base,
                       fsehip_stream_t stream);

/* fsehip_planes_compress with the diff image against d_base in place of the
 * plane image: the same arguments, alignment rules (d_src and d_base to
 * elem_bytes, d_scratch to 16, d_out any), capacities
 * (fsehip_diff_scratch_bytes, fsehip_diff_bound) and statuses, UNSUPPORTED for
 * elem_bytes outside {1, 2, 4, 8}; nothing allocated for the transform, no
 * host synchronisation. */
int fsehip_diff_compress(const fsehip_frame_params* p, uint32_t elem_bytes, const void* d_src, const void* d_base,
                         uint64_t n_elems, uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
                         uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream);

/* fsehip_planes_decompress for a diff frame whose first 48 bytes
 * fsehip_diff_read_header parsed into `info` and `inner`, against the
 * info->n_elems elements at d_base: the same arguments, rules and statuses
 * (d_out 16-byte aligned; d_base itself, the in-place decode, or clear of
 * it); on BAD_FRAME every block status is BAD_FRAME and no byte of d_out is
 * touched.  A failed inner block costs the elements with a byte in it; every
 * other element is exact. */
int fsehip_diff_decompress(const fsehip_diff_info* info, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                           const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap,
                           void* d_out, const void* d_base, uint64_t out_cap, int32_t* d_block_status,
                           int32_t* d_result, fsehip_stream_t stream);

/* The scratch fsehip_diff_decompress_ranges needs for a range list (host
 * array): fsehip_planes_ranges_scratch_bytes' formula, at elem_bytes 1 too.
 * 0 for a bad elem_bytes or on overflow. */
uint64_t fsehip_diff_ranges_scratch_bytes(uint32_t elem_bytes, const fsehip_planes_range* ranges, uint32_t n_ranges);

/* fsehip_planes_decompress_ranges for a diff frame: a range maps to the w
 * byte ranges of the inner frame a plane range maps to, and its base elements
 * are d_base[elem_off .. elem_off + n_elems) -- d_base points at the whole
 * base tensor, info->n_elems elements, whatever the ranges.  The range rules,
 * statuses and argument checks are those of fsehip_planes_decompress_ranges,
 * with fsehip_diff_ranges_scratch_bytes for the scratch; and BAD_ARG for a
 * null d_base with a non-empty range, one not aligned to elem_bytes, or any
 * overlap of d_out's bytes up to the end of the last destination with the
 * base. */
int fsehip_diff_decompress_ranges(const fsehip_diff_info* info, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                                  const uint8_t* d_in, uint64_t in_len, const fsehip_planes_range* ranges,
                                  uint32_t n_ranges, uint8_t* d_scratch, uint64_t scratch_cap, void* d_out,
                                  const void* d_base, uint64_t out_cap, int32_t* d_range_status, int32_t* d_result,
                                  fsehip_stream_t stream);

/* ------------------------------------------------------------------------
 * (2i) Size estimates with a base: the diff frame as fourth kind
 *
 * A caller who holds the tensor's previous version can have a diff frame
 * (section 2h); whether it pays depends on how close the two are (DESIGN.md
 * section 5 "Estimate": a fifth of the plane frame after a small step, 5 %
 * more than it for unrelated tensors).  Once the caller hands the base over,
 * that is again something a histogram finds: the diff image's block counts,
 * taken from the two sources without writing the image, through the block
 * rule of section 2g unchanged.  A diff frame: 16 + the frame estimate of its
 * image.  No format changes, and the calls of section 2g stay as they are:
 * kinds above 2 are theirs to refuse.
 * ------------------------------------------------------------------------ */

/* fsehip_image_histogram for the diff image (section 2h) of the n_elems
 * elements of elem_bytes (1, 2, 4, 8) at d_src against those at d_base: the
 * counts of its ceil(elem_bytes * roundup(n_elems, 16) / block_size) blocks,
 * zeroed by the call and then added to.  Both sources are read once, aligned
 * to elem_bytes each on its own, up to roundup(n_elems * elem_bytes, 4) at
 * most; they may overlap in any way or be one pointer (every count then in
 * bin 0).  Nothing but d_counts is written.  Asynchronous on `stream`, no
 * host synchronisation, no workspace.  Before any device use: UNSUPPORTED
 * (elem_bytes outside {1, 2, 4, 8}, a size overflowing), BAD_ARG (a null or
 * misaligned d_src, d_base or d_counts with n_elems > 0, more than one block
 * of a size that is no multiple of 16, more than 2^32 - 1 blocks), NO_DEVICE.
 * n_elems == 0 returns FSE_OK and does nothing. */
int fsehip_diff_image_histogram(uint32_t elem_bytes, const void* d_src, const void* d_base, uint64_t n_elems,
                                uint32_t block_size, uint32_t* d_counts, fsehip_stream_t stream);

/* fsehip_estimate_scratch_bytes for a kind_mask of bits 0, 1, 2 (as there)
 * and 4 (FSEHIP_KIND_DIFF, whose image has the delta image's size).  0 for a
 * kind_mask of 0, with bit 3 or any bit above 4, and as there. */
uint64_t fsehip_estimate_base_scratch_bytes(uint64_t n_elems, uint32_t elem_bytes, uint32_t kind_mask,
                                            uint32_t block_size);

/* fsehip_estimate with the diff frame against d_base as a further kind:
 * kind_mask has bits 0, 1, 2 and 4, and d_est is FIVE u64 on the device,
 * indexed by FSEHIP_KIND_*.  d_est[3] (a sealed buffer is no choice of
 * container) is always FSEHIP_EST_NONE; d_est[4] = 16 + 32 + 4 * n_blocks +
 * the sum of rec over the diff image's blocks, 48 for n_elems = 0, or
 * FSEHIP_EST_NONE when bit 4 is clear.  With bit 4 clear d_est[0..2] are what
 * fsehip_estimate gives for the same mask, and d_base is ignored; with bit 4
 * set and n_elems > 0 a null d_base, or one not aligned to elem_bytes, is
 * BAD_ARG.  A kind_mask of 0, with bit 3 or with any bit above 4 is BAD_ARG;
 * d_scratch is fsehip_estimate_base_scratch_bytes; every other rule, status
 * and promise (one scratch, the kinds one after the other, asynchronous, no
 * workspace, no host synchronisation) is fsehip_estimate's. */
int fsehip_estimate_base(const fsehip_frame_params* p, uint32_t kind_mask, uint32_t elem_bytes, const void* d_src,
                         const void* d_base, uint64_t n_elems, uint8_t* d_scratch, uint64_t scratch_bytes,
                         uint64_t* d_est, fsehip_stream_t stream);

/* Host function, no device: the kind of the smallest entry of est[5] (indexed
 * by FSEHIP_KIND_*).  Ties go to the frame, then the plane frame, then the
 * delta frame, then the diff frame: a container that needs its base to decode
 * wins only when strictly smaller.  est[3] and entries of FSEHIP_EST_NONE do
 * not take part; -1 when nothing is left or est is null. */
int fsehip_estimate_choose_base(const uint64_t est[5]);

/* ------------------------------------------------------------------------
 * (2j) Pack frames: many tensors in one container, one call each way
 *
 * The containers of sections 2b, 2d, 2e and 2h take one tensor per call.  A
 * checkpoint, a state_dict or a set of CSR arrays is hundreds or thousands of
 * tensors, most of them small; a caller's loop pays launches, a 48-byte head
 * and a table header per tensor, and a 2 KiB tensor is one workgroup.  The
 * pack frame takes the whole list: one transform launch over all members,
 * one unchanged frame of section 2b over one image, one launch back.  This
 * library's own container, version 1; integers little-endian, no padding, any
 * byte address:
 *
 *   header, 32 bytes
 *    0  u8[4] magic "FSEM"
 *    4  u8    version = 1
 *    5  u8[3] reserved = 0
 *    8  u32   n_members       0 .. FSEHIP_PACK_MAX_MEMBERS
 *   12  u32   reserved = 0
 *   16  u64   image_bytes     = sum over members of w_m * stride_m (= the inner frame's n_total)
 *   24  u64   content_bytes   = sum over members of w_m * n_m
 *   member table, n_members x 16 bytes
 *    0  u8    kind            FSEHIP_KIND_PLANES or FSEHIP_KIND_DELTA
 *    1  u8    elem_bytes w    1, 2, 4 or 8 for either kind (planes at w = 1: the bytes themselves)
 *    2  u8[6] reserved = 0
 *    8  u64   n_elems         0 is valid
 *   one frame (section 2b) of the image, to the end of the buffer
 *
 * The image.  stride_m = roundup(n_m, 16).  z_m is member m's elements for
 * the plane kind, and for the delta kind the zigzag deltas of section 2e with
 * a restart every FSEHIP_DELTA_RESTART elements counted from the member's own
 * element 0.  Plane k of member m is byte k of every element of z_m: stride_m
 * bytes, the pad zero.  The image is segments 0..7 back to back, plane-major
 * from the top byte: segment j holds, for each member with w_m > j in member
 * order, that member's plane w_m - 1 - j.  So every member's sign/exponent
 * bytes (or zero high bytes) sit together, then every member's next byte, and
 * a block's one table never averages a small tensor's exponent plane with its
 * mantissa plane.  Every plane starts at a multiple of 16.
 *
 * A reader rejects (BAD_FRAME) any nonzero reserved byte, another version, a
 * kind or width outside the lists, n_members above the cap, sums that
 * overflow or differ from the two header fields, and an inner n_total other
 * than image_bytes.  "FSEM" is BAD_FRAME to every other reader of this header
 * (fsehip_sealed_read_header included) and their magics are BAD_FRAME here.
 *
 * As the other element frames, the container stores neither names, dtypes,
 * shapes nor bases.  Diff members (section 2h) live in the versioned pack of
 * section 2k, and sealing a pack is the member check record of section 2l.
 * A per-member automatic kind (section 2g) is out of scope of version 1; the
 * kind byte and the reserved fields leave room for it.
 *
 * A failed inner block costs the elements with a byte in it, and for a delta
 * member the rest of that restart group as well; BAD_FRAME stores nothing to
 * any member.
 * ------------------------------------------------------------------------ */
#define FSEHIP_KIND_PACK 5u /* section 2j, magic "FSEM": fsehip_container_kind only */
#define FSEHIP_PACK_MAX_MEMBERS (1u << 20)

/* One member: n_elems elements of elem_bytes at d_ptr (device memory, aligned
 * to elem_bytes; ignored for n_elems = 0 and by the host calls), coded as
 * kind.  The encoder reads up to roundup(n_elems * elem_bytes, 4) bytes of
 * each member at most; the decoders store exactly n_elems * elem_bytes. */
typedef struct fsehip_pack_member {
    void* d_ptr;
    uint64_t n_elems;
    uint32_t elem_bytes;
    uint32_t kind;
} fsehip_pack_member;

typedef struct fsehip_pack_info {
    uint32_t version;
    uint32_t n_members;
    uint64_t image_bytes;
    uint64_t content_bytes;
} fsehip_pack_info;

/* Host functions, no device.  A list is valid with at most
 * FSEHIP_PACK_MAX_MEMBERS members, kinds and widths of the lists above and
 * sums that fit 64 bits.
 *  fsehip_pack_image_bytes: the image's size (0 for an invalid list, and for
 *    one without elements).
 *  fsehip_pack_bound: an output capacity that holds the pack at that block
 *    size, 32 + 16 n + fsehip_frame_bound(image); 0 for an invalid list.
 *  fsehip_pack_scratch_bytes: the scratch of fsehip_pack_compress and
 *    fsehip_pack_decompress (the image, the members' descriptors, the head);
 *    minus fsehip_pack_image_bytes: that of the two bare transforms.  0 for an
 *    invalid list.
 *  fsehip_pack_members_scratch_bytes: that of fsehip_pack_decompress_members
 *    for the members sel[0 .. n_sel); 0 for an invalid list or a selection out
 *    of range.
 *  fsehip_pack_plane_offset: where byte k of member m's elements lies in the
 *    image; UINT64_MAX for an invalid list, m or k. */
uint64_t fsehip_pack_image_bytes(const fsehip_pack_member* members, uint32_t n_members);
uint64_t fsehip_pack_bound(const fsehip_pack_member* members, uint32_t n_members, uint32_t block_size);
uint64_t fsehip_pack_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members);
uint64_t fsehip_pack_members_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members, const uint32_t* sel,
                                           uint32_t n_sel);
uint64_t fsehip_pack_plane_offset(const fsehip_pack_member* members, uint32_t n_members, uint32_t m, uint32_t k);

/* Host functions, no device.  fsehip_pack_read_header parses the first 32
 * bytes (the table's length follows from n_members: 16 each); BAD_FRAME and
 * *out zeroed for fewer bytes or a broken rule.  fsehip_pack_read_members
 * parses the header, the table and the inner frame's header from the
 * 32 + 16 n + 32 bytes at buf: members[m] gets kind, elem_bytes and n_elems
 * (d_ptr null), *out and *inner the two headers; DST_TOO_SMALL when
 * members_cap is below n_members, BAD_FRAME (outputs zeroed) for every rule
 * above.  fsehip_pack_write_header writes the 32 + 16 n head bytes of a valid
 * list (BAD_ARG otherwise). */
int fsehip_pack_read_header(const uint8_t* buf, size_t len, fsehip_pack_info* out);
int fsehip_pack_read_members(const uint8_t* buf, size_t len, fsehip_pack_member* members, uint32_t members_cap,
                             fsehip_pack_info* out, fsehip_frame_info* inner);
int fsehip_pack_write_header(const fsehip_pack_member* members, uint32_t n_members, uint8_t* out);

/* The bare transforms: every member's elements into the image at d_image
 * (16-byte aligned, fsehip_pack_image_bytes) and back, one launch for all
 * members.  d_scratch (16-byte aligned, fsehip_pack_scratch_bytes minus the
 * image) takes the members' descriptors, which reach the device through the
 * stream's pinned staging: asynchronous on `stream`, no host synchronisation.
 * A member's pointer is aligned to its elements, for the split as
 * fsehip_planes_split; the merge stores at that alignment too (members are
 * carved from arenas), exactly n_elems * elem_bytes bytes each, and its
 * destinations must not overlap.  Before any device use: UNSUPPORTED (an
 * invalid list), BAD_ARG (a null or misaligned pointer with elements,
 * overlapping destinations), DST_TOO_SMALL (the scratch), NO_DEVICE.  A list
 * without elements returns FSE_OK and does nothing. */
int fsehip_pack_split(const fsehip_pack_member* members, uint32_t n_members, uint8_t* d_image, uint8_t* d_scratch,
                      uint64_t scratch_cap, fsehip_stream_t stream);
int fsehip_pack_merge(const fsehip_pack_member* members, uint32_t n_members, const uint8_t* d_image,
                      uint8_t* d_scratch, uint64_t scratch_cap, fsehip_stream_t stream);

/* The pack of the members at d_out: the split, one fsehip_frame_compress of
 * the image in d_scratch (16-byte aligned, fsehip_pack_scratch_bytes; needed
 * for an empty list too), then the header and the table written on the
 * device.  *d_out_len = the pack's bytes, d_result as fsehip_frame_compress.
 * Asynchronous, no host synchronisation.  Before any device use: BAD_ARG (a
 * null pointer, a member pointer null or misaligned with elements, the frame
 * parameters' rules), UNSUPPORTED (an invalid list, a block above the limit),
 * DST_TOO_SMALL (scratch_cap or out_cap below fsehip_pack_bound), NO_DEVICE. */
int fsehip_pack_compress(const fsehip_frame_params* p, const fsehip_pack_member* members, uint32_t n_members,
                         uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out, uint64_t out_cap,
                         uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream);

/* Decode the pack at d_in into the members' destinations: `info`, the
 * members' fields and `inner` are what fsehip_pack_read_members gave, with
 * d_ptr set (info->n_members members).  One fsehip_frame_decompress into
 * d_scratch (fsehip_pack_scratch_bytes), a device check of the 32 + 16 n head
 * bytes against the caller's, one merge.  d_block_status (may be NULL) and
 * d_result are the inner frame call's; a head on the device that differs from
 * the caller's is BAD_FRAME in d_result[0] and every block status, and stores
 * nothing.  Before any device use: BAD_ARG (a null pointer, members that do
 * not sum to `info` or `inner`, a destination null, misaligned or overlapping
 * another), UNSUPPORTED (an invalid list), DST_TOO_SMALL (the scratch),
 * NO_DEVICE. */
int fsehip_pack_decompress(const fsehip_pack_info* info, const fsehip_pack_member* members,
                           const fsehip_frame_info* inner, uint32_t chunk_blocks, const uint8_t* d_in, uint64_t in_len,
                           uint8_t* d_scratch, uint64_t scratch_cap, int32_t* d_block_status, int32_t* d_result,
                           fsehip_stream_t stream);

/* Decode only the members sel[0 .. n_sel) (indices into the list, each once,
 * any order): their plane ranges go through ONE
 * fsehip_frame_decompress_ranges call into d_scratch
 * (fsehip_pack_members_scratch_bytes), so only the blocks they cover are
 * decoded, then one merge.  Only the selected members need a d_ptr; the
 * others' destinations are never touched.  d_member_status[s] (may be NULL)
 * is the status of member sel[s]: its first failing plane range's, FSE_OK for
 * a member without elements, BAD_FRAME for all on a bad head; d_result[0] is
 * the frame's status and d_result[1] the members with a status.  Checks as
 * fsehip_pack_decompress, and BAD_ARG for a selection out of range or named
 * twice. */
int fsehip_pack_decompress_members(const fsehip_pack_info* info, const fsehip_pack_member* members,
                                   const fsehip_frame_info* inner, uint32_t chunk_blocks, const uint8_t* d_in,
                                   uint64_t in_len, const uint32_t* sel, uint32_t n_sel, uint8_t* d_scratch,
                                   uint64_t scratch_cap, int32_t* d_member_status, int32_t* d_result,
                                   fsehip_stream_t stream);

/* ------------------------------------------------------------------------
 * (2k) Versioned pack: diff members against base tensors in a pack frame
 *
 * The next checkpoint against the previous one is every tensor of a
 * state_dict against its predecessor: the diff frame of section 2h per
 * tensor, the pack frame of section 2j for the list.  The versioned pack is
 * both at once: a sibling of the pack frame with its own magic, over the same
 * host code and the same tile kernels, whose member kind list gains the diff
 * kind.  This is where the diff members that section 2j leaves out live.
 *
 * The layout is byte for byte that of section 2j (a 32-byte header, 16 bytes
 * per member, one unchanged frame of section 2b over one image, planes
 * plane-major from the top byte, every plane padded to 16) with
 *    magic "FSEV", version = 1
 *    kind  FSEHIP_KIND_PLANES, FSEHIP_KIND_DELTA or FSEHIP_KIND_DIFF
 * For a diff member, z_m is the zigzag difference of section 2h of the
 * member's elements against its base's, a tensor of the same width and count:
 * z_i = zigzag(x_i - b_i) mod 2^(8 w), no restarts.  Planes and delta members
 * are exactly as in 2j, so a versioned pack without a diff member differs
 * from the pack frame of the same list in its magic only.
 *
 * THE CONTAINER DOES NOT IDENTIFY ITS BASES.  As with the diff frame, a
 * decode against another base of the same size succeeds with every status
 * FSE_OK and yields other values; which tensor a member was coded against is
 * the caller's to know (a checkpoint step, a content hash beside the pack) --
 * or the sealed pack's of section 2l, whose record holds every base's CRC-32
 * and whose decode verifies the bases before it stores a byte.
 *
 * The reader rules are those of 2j: BAD_FRAME for any nonzero reserved byte,
 * another version, a kind outside {1, 2, 4} or a width outside the list,
 * n_members above the cap, sums that overflow or differ from the two header
 * fields, and an inner n_total other than image_bytes.  "FSEV" is BAD_FRAME to
 * every other reader of this header (the frame, planes, delta, diff and check
 * readers, fsehip_sealed_read_header, fsehip_pack_read_header and
 * fsehip_pack_read_members) and their magics are BAD_FRAME here.
 *
 * A versioned pack is sealed by the member check record of section 2l.  Out
 * of scope of version 1: a per-member automatic kind (section 2i), element
 * ranges inside a member.
 *
 * A failed inner block costs the elements with a byte in it, and for a delta
 * member the rest of that restart group as well; for a diff member decoded in
 * place the base's values there are lost too.  BAD_FRAME stores nothing to
 * any member.
 * ------------------------------------------------------------------------ */
#define FSEHIP_KIND_VPACK 6u /* section 2k, magic "FSEV": fsehip_container_kind only */

/* The calls mirror fsehip_pack_* one for one over the same fsehip_pack_member
 * list (kind may be FSEHIP_KIND_DIFF) and fsehip_pack_info.  The host calls
 * are those of section 2j for this container's magic and kinds;
 * fsehip_vpack_scratch_bytes and fsehip_vpack_members_scratch_bytes also hold
 * one base pointer per member. */
uint64_t fsehip_vpack_image_bytes(const fsehip_pack_member* members, uint32_t n_members);
uint64_t fsehip_vpack_bound(const fsehip_pack_member* members, uint32_t n_members, uint32_t block_size);
uint64_t fsehip_vpack_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members);
uint64_t fsehip_vpack_members_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members, const uint32_t* sel,
                                            uint32_t n_sel);
uint64_t fsehip_vpack_plane_offset(const fsehip_pack_member* members, uint32_t n_members, uint32_t m, uint32_t k);
int fsehip_vpack_read_header(const uint8_t* buf, size_t len, fsehip_pack_info* out);
int fsehip_vpack_read_members(const uint8_t* buf, size_t len, fsehip_pack_member* members, uint32_t members_cap,
                              fsehip_pack_info* out, fsehip_frame_info* inner);
int fsehip_vpack_write_header(const fsehip_pack_member* members, uint32_t n_members, uint8_t* out);

/* The device calls are those of section 2j with `d_bases` behind the member
 * list: a HOST array of n_members device pointers, d_bases[m] the base of
 * member m (n_elems elements of elem_bytes, aligned to elem_bytes).  An entry
 * is ignored for planes and delta members and for members without elements;
 * the array may be NULL when no member with elements is a diff member.
 * fsehip_vpack_decompress_members needs the bases of the selected diff
 * members only.  The pointers travel to the device with the descriptors and
 * the head in the one copy through the stream's pinned staging: every call is
 * asynchronous on `stream`, no host synchronisation.
 *
 * Reads: up to roundup(n_elems * elem_bytes, 4) bytes of a source and of a
 * base, as fsehip_diff_*.  Stores: exactly n_elems * elem_bytes bytes per
 * member, at element alignment.
 *
 * Before any device use, the checks of the fsehip_pack_* call, and: a diff
 * member with elements whose base is NULL or not aligned to its elements is
 * BAD_ARG.  On the decode side (merge, decompress, decompress_members) a diff
 * member's destination may be its base itself (d_ptr == d_bases[m]: the
 * in-place update of a checkpoint); any other overlap of a destination with
 * another destination or with the base of a decoded diff member, counting
 * only members with elements, is BAD_ARG.  On the split side bases and
 * sources are only read and may overlap. */
int fsehip_vpack_split(const fsehip_pack_member* members, uint32_t n_members, const void* const* d_bases,
                       uint8_t* d_image, uint8_t* d_scratch, uint64_t scratch_cap, fsehip_stream_t stream);
int fsehip_vpack_merge(const fsehip_pack_member* members, uint32_t n_members, const void* const* d_bases,
                       const uint8_t* d_image, uint8_t* d_scratch, uint64_t scratch_cap, fsehip_stream_t stream);
int fsehip_vpack_compress(const fsehip_frame_params* p, const fsehip_pack_member* members, uint32_t n_members,
                          const void* const* d_bases, uint8_t* d_scratch, uint64_t scratch_cap, uint8_t* d_out,
                          uint64_t out_cap, uint64_t* d_out_len, int32_t* d_result, fsehip_stream_t stream);
int fsehip_vpack_decompress(const fsehip_pack_info* info, const fsehip_pack_member* members,
                            const void* const* d_bases, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                            const uint8_t* d_in, uint64_t in_len, uint8_t* d_scratch, uint64_t scratch_cap,
                            int32_t* d_block_status, int32_t* d_result, fsehip_stream_t stream);
int fsehip_vpack_decompress_members(const fsehip_pack_info* info, const fsehip_pack_member* members,
                                    const void* const* d_bases, const fsehip_frame_info* inner, uint32_t chunk_blocks,
                                    const uint8_t* d_in, uint64_t in_len, const uint32_t* sel, uint32_t n_sel,
                                    uint8_t* d_scratch, uint64_t scratch_cap, int32_t* d_member_status,
                                    int32_t* d_result, fsehip_stream_t stream);

/* ------------------------------------------------------------------------
 * (2l) Sealed pack: per-member CRC-32 of contents and bases, verified on device
 *
 * The check record of section 2f covers one contiguous content, and a pack's
 * members lie wherever the caller's tensors do; a versioned pack decoded
 * against the wrong previous checkpoint returns wrong weights with every block
 * status FSE_OK, and in place it has overwritten the old checkpoint by then.
 * The member check record holds one CRC-32 per member's content and, for diff
 * members, one per base; they are computed over all members in a constant
 * number of launches, travel in front of an unchanged pack, and on decode the
 * bases are verified BEFORE the merge may store a byte, the destinations
 * after it.  This library's own record, version 1; integers little-endian, no
 * padding, any byte address:
 *
 *   header, 32 bytes
 *    0  u8[4] magic "FSES"
 *    4  u8    version = 1
 *    5  u8    algorithm = 1 (FSEHIP_CHECK_CRC32)
 *    6  u8    flags: bit 0 (FSEHIP_MCHECK_BASES) = base CRCs recorded; other bits 0
 *    7  u8    0
 *    8  u32   n_members
 *   12  u32   reserved = 0
 *   16  u64   content_bytes   (= the pack's content_bytes)
 *   24  u32   reserved = 0
 *   28  u32   header_crc      CRC-32 of bytes 0..27
 *   table, n_members x 8 bytes
 *    0  u32   content_crc     CRC-32 (zlib's) of the member's n_elems * w bytes; 0 when empty
 *    4  u32   base_crc        CRC-32 of the base's n_elems * w bytes for a diff member with
 *                             elements when flag bit 0 is set; otherwise 0
 *
 * A sealed pack is this record followed directly by exactly one pack frame
 * ("FSEM", section 2j) or versioned pack ("FSEV", section 2k), to the end of
 * the buffer; the inner container's bytes are unchanged.  The record's
 * n_members and content_bytes equal the pack's, and flag bit 0 is valid only
 * in front of "FSEV"; a reader rejects (BAD_FRAME) anything else, any nonzero
 * reserved byte, another version or algorithm and a wrong header_crc.  "FSES"
 * is BAD_FRAME to every other reader and their magics are BAD_FRAME here.  The
 * record's size, 32 + 8 n, is known before anything runs, so the pack is
 * compressed straight to its final place.
 *
 * The table is deliberately not covered by a CRC of its own: a damaged entry
 * shows as CHECKSUM of that member, or as a failed base -- both the safe
 * direction.  Granularity is the member, the unit fsehip_pack_decompress_members
 * reports, not section 2f's 64 KiB: a selected-member decode verifies whole
 * members, with none of section 2f's partial-block caveat.
 *
 * The gate is all or nothing: one base that fails its CRC (or a record header
 * on the device that differs from the caller's) and the merge stores nothing
 * to any member, in place or not -- the right rule for a checkpoint update.
 * ------------------------------------------------------------------------ */
#define FSEHIP_KIND_SPACK 7u /* section 2l, magic "FSES": fsehip_container_kind only */
#define FSEHIP_MCHECK_BASES 1u /* flags bit 0: the table's base CRCs are recorded */

typedef struct fsehip_mcheck_info {
    uint32_t version;
    uint32_t algorithm; /* FSEHIP_CHECK_CRC32 */
    uint32_t flags;     /* FSEHIP_MCHECK_BASES or 0 */
    uint32_t n_members;
    uint64_t content_bytes;
    uint32_t header_crc;
    uint32_t reserved; /* 0 */
} fsehip_mcheck_info;

/* Host functions, no device.
 *  fsehip_mcheck_bytes: the record's size, 32 + 8 n; 0 above
 *    FSEHIP_PACK_MAX_MEMBERS.
 *  fsehip_mcheck_read_header: parses 32 bytes; BAD_FRAME and *out zeroed for
 *    fewer bytes or a broken rule.  fsehip_mcheck_write_header: the 32 bytes of
 *    valid fields (header_crc is computed, not read); BAD_ARG otherwise.
 *  fsehip_spack_read_header: the record's header of a sealed pack, whether the
 *    pack behind it is versioned, and where it starts (hand buf + *inner_off to
 *    fsehip_pack_read_members or fsehip_vpack_read_members); BAD_FRAME with
 *    every output zeroed for any rule above.
 *  fsehip_mcheck_scratch_bytes: the scratch of fsehip_mcheck_build (sel NULL,
 *    with_bases as d_bases is given) and of fsehip_mcheck_verify (the members
 *    sel[0 .. n_sel), or all for sel NULL; with_bases 0); 0 for an invalid list
 *    or selection.
 *  fsehip_spack_bound, fsehip_spack_scratch_bytes,
 *  fsehip_spack_members_scratch_bytes: as fsehip_pack_* / fsehip_vpack_*
 *    (`versioned` says which) plus the record and the check kernels' scratch. */
uint64_t fsehip_mcheck_bytes(uint32_t n_members);
int fsehip_mcheck_read_header(const uint8_t* hdr, size_t len, fsehip_mcheck_info* out);
int fsehip_mcheck_write_header(const fsehip_mcheck_info* info, uint8_t hdr[32]);
int fsehip_spack_read_header(const uint8_t* buf, size_t len, fsehip_mcheck_info* info, uint32_t* versioned,
                             uint64_t* inner_off);
uint64_t fsehip_mcheck_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members, const uint32_t* sel,
                                     uint32_t n_sel, uint32_t with_bases);
uint64_t fsehip_spack_bound(const fsehip_pack_member* members, uint32_t n_members, uint32_t versioned,
                            uint32_t block_size);
uint64_t fsehip_spack_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members, uint32_t versioned);
uint64_t fsehip_spack_members_scratch_bytes(const fsehip_pack_member* members, uint32_t n_members, uint32_t versioned,
                                            const uint32_t* sel, uint32_t n_sel);

/* The record of the members as they lie, to d_record (any address,
 * fsehip_mcheck_bytes): content CRCs of every member at its d_ptr and, with
 * d_bases (a HOST array of device pointers as in section 2k; NULL: none, flag
 * bit 0 clear), the base CRCs of the diff members.  Three launches whatever n:
 * one CRC per 64 KiB work unit of every span, the units combined per span, the
 * table and header written.  d_scratch: 16-byte aligned,
 * fsehip_mcheck_scratch_bytes.  Members are read at element alignment: whole
 * aligned 16-byte words that hold a content byte, never more.  Asynchronous on
 * `stream`, no host synchronisation.  Before any device use: BAD_ARG (a null
 * pointer, a member or base null or misaligned with elements), UNSUPPORTED (an
 * invalid list), DST_TOO_SMALL (the scratch), NO_DEVICE. */
int fsehip_mcheck_build(const fsehip_pack_member* members, const void* const* d_bases, uint32_t n_members,
                        uint8_t* d_record, uint8_t* d_scratch, uint64_t scratch_cap, fsehip_stream_t stream);

/* Verify spans against the record at d_record, whose header `info` the caller
 * has read: the members sel[0 .. n_sel) (each once), or all info->n_members
 * for sel NULL.  which = 0: the member's n_elems * w bytes at d_ptrs[m] (a
 * HOST array indexed by member; NULL: at members[m].d_ptr) against
 * content_crc.  which = 1: a diff member's base at d_ptrs[m] against base_crc;
 * without FSEHIP_MCHECK_BASES in info->flags nothing is read and every status
 * is FSE_OK.  d_status[s] = FSE_OK or FSE_ERR_CHECKSUM per span, d_result[0] =
 * FSE_OK, FSE_ERR_CHECKSUM when one failed, or FSE_ERR_BAD_FRAME (every status
 * too) when the header on the device differs from `info`; d_result[1] = the
 * spans that failed.  Asynchronous, three launches.  Checks as
 * fsehip_mcheck_build, and BAD_ARG for members that do not sum to
 * info->content_bytes or a selection out of range or named twice. */
int fsehip_mcheck_verify(const fsehip_mcheck_info* info, const uint8_t* d_record, const fsehip_pack_member* members,
                         const uint32_t* sel, uint32_t n_sel, uint32_t which, const void* const* d_ptrs,
                         uint8_t* d_scratch, uint64_t scratch_cap, int32_t* d_status, int32_t* d_result,
                         fsehip_stream_t stream);

/* The sealed pack of the members at d_out: fsehip_pack_compress, or with
 * d_bases fsehip_vpack_compress, straight to d_out + 32 + 8 n, then the
 * record in front of it; with d_bases and check_bases the base CRCs are
 * recorded.  *d_out_len includes the record.  d_scratch:
 * fsehip_spack_scratch_bytes; out_cap: fsehip_spack_bound.  Statuses as the
 * pack call's. */
int fsehip_spack_compress(const fsehip_frame_params* p, const fsehip_pack_member* members, uint32_t n_members,
                          const void* const* d_bases, uint32_t check_bases, uint8_t* d_scratch, uint64_t scratch_cap,
                          uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_len, int32_t* d_result,
                          fsehip_stream_t stream);

/* Decode the sealed pack at d_in (the record first; in_len the whole buffer).
 * `rec`, `versioned` are fsehip_spack_read_header's, `info`, the members'
 * fields and `inner` those of the pack reader at buf + inner_off; the other
 * arguments are the pack call's.  d_member_check / d_base_check: one int32
 * per member (per selected member), either may be NULL.  d_check_result[4]:
 *   [0] FSE_OK, FSE_ERR_CHECKSUM when any verified member or base failed, or
 *       FSE_ERR_BAD_FRAME when the record's header on the device differs from
 *       the caller's (then every check status too)
 *   [1] members whose content failed   [2] members whose base failed   [3] 0
 * Order on the stream: the bases verified; the frame decoded into scratch; the
 * pack head checked; the gate; the merge; the destinations verified.  The
 * merge stores nothing when d_result[0] is BAD_FRAME, when a base failed or
 * when the record's header differs.  Content verification always runs: its
 * statuses say truthfully whether destination m holds the recorded content --
 * after a closed gate, CHECKSUM wherever the new content differs from what
 * lies there.  A buffer sealed without base CRCs decodes with every base
 * status FSE_OK; a wrong base then shows as the member's CHECKSUM after the
 * merge.  Asynchronous, no host synchronisation, a constant number of launches
 * beyond the pack call's.  Before any device use: the pack call's statuses,
 * and BAD_ARG for a record that does not agree with `info` or `versioned`. */
int fsehip_spack_decompress(const fsehip_mcheck_info* rec, const fsehip_pack_info* info, uint32_t versioned,
                            const fsehip_pack_member* members, const void* const* d_bases,
                            const fsehip_frame_info* inner, uint32_t chunk_blocks, const uint8_t* d_in, uint64_t in_len,
                            uint8_t* d_scratch, uint64_t scratch_cap, int32_t* d_block_status, int32_t* d_result,
                            int32_t* d_member_check, int32_t* d_base_check, int32_t* d_check_result,
                            fsehip_stream_t stream);
int fsehip_spack_decompress_members(const fsehip_mcheck_info* rec, const fsehip_pack_info* info, uint32_t versioned,
                                    const fsehip_pack_member* members, const void* const* d_bases,
                                    const fsehip_frame_info* inner, uint32_t chunk_blocks, const uint8_t* d_in,
                                    uint64_t in_len, const uint32_t* sel, uint32_t n_sel, uint8_t* d_scratch,
                                    uint64_t scratch_cap, int32_t* d_member_status, int32_t* d_result,
                                    int32_t* d_member_check, int32_t* d_base_check, int32_t* d_check_result,
                                    fsehip_stream_t stream);

/* ------------------------------------------------------------------------
 * (2c) Shared-table coding: many small messages against one caller's table
 *
 * The crate's `pub mod fse` lets a caller code any number of messages against
 * one table, with no header in front: EncodeTable::new(&NormHistogram),
 * Encoder::{new_first_symbol, encode_raw, encode, finish}, DecodeTable::new,
 * Decoder::{new, decode_symbol, finish} (fse.rs:86-386; its own tests do so,
 * fse.rs:394-434).  Here that is one table image on the device and two
 * batched calls.  There is no new format -- a message's payload is
 *   nstates 2: the body of fse_compress2 from BitStackWriter::new on
 *              (lib.rs:151-182), decoded by the loop of lib.rs:222-247;
 *   nstates 1: the headerless stream of fse.rs:394-421 (= lib.rs:118-142),
 *              decoded by the loop of lib.rs:187-211;
 * so with the message's own normalised histogram as the table, the payload is
 * the crate's stream minus its header bytes.  Small records gain twice: no
 * table build and no header per message (a 512-byte message against a table
 * trained on a sample: DESIGN.md section 5).
 * ------------------------------------------------------------------------ */

/* `impl TryFrom<[i32; 256]> for NormHistogram` (histogram.rs:508-536), with
 * its quirks: the sum of |x| must be a power of two (log2 of it is the table
 * log, whatever its value -- a log outside 5..15 is refused later, by the
 * table build), and table_len = 1 + the last non-zero index.  Err(()) and the
 * all-zero table (the crate's 0.ilog2() panic) are FSE_ERR_BAD_TABLE.  Host
 * only, no device. */
int norm_histogram_try_from(const int32_t table[256], fse_norm_histogram* out);

/* EncodeTable::new + DecodeTable::new (fse.rs:88-189, 269-338) of the
 * NormHistogram at d_nh (device memory) as one opaque image of
 * fsehip_shared_table_bytes() bytes at d_table (16-byte aligned): the encode
 * stateTable and symbol transforms, the decode table, which symbols have a
 * slot, the table log and a validity word.  Table logs 5..12.  *d_status:
 * FSE_OK; UNSUPPORTED for a log of 13..15; TABLELOG_RANGE outside 5..15;
 * BAD_TABLE for table_len outside 1..256, an entry below -1, counts (-1 as 1)
 * that do not sum to 2^log2 or a spread that does not close (fse.rs:151 /
 * 326).  A failed build leaves the image marked invalid: every message coded
 * with it gets BAD_TABLE and nothing is indexed with its contents.  The image
 * may be copied and used on any stream after the build.  Asynchronous; BAD_ARG
 * (a null or misaligned pointer) and NO_DEVICE before any device use. */
uint64_t fsehip_shared_table_bytes(void);
int fsehip_shared_table_build(const fse_norm_histogram* d_nh, uint8_t* d_table, int32_t* d_status,
                              fsehip_stream_t stream);

/* An output capacity that holds the payload of any message of src_len bytes
 * at that table log (clamped to 5..12): src_len * L + 2 L + 1 bits, rounded
 * up to 16 bytes. */
uint64_t fsehip_shared_out_bytes(uint32_t src_len, uint32_t table_log);

/* Encode n_msgs messages against the image d_table, one lane per message.
 * Message i is the src_len bytes at d_src + src_off; its payload goes to
 * d_out + out_off, at most out_cap bytes (fsehip_stream_desc and the memory
 * rules of fsehip_compress_streams: reads are exactly [src_off, src_off +
 * src_len); stores only inside [out_off, out_off + out_cap), whatever the
 * status; bytes of a region beyond d_comp_len[i] are unspecified; regions do
 * not overlap; d_table, d_src and d_out 16-byte aligned).
 * d_comp_len[i] = payload bytes, d_payload_bits[i] (may be NULL) = its bits
 * with the marker (the crate's return value); both 0 for a message that
 * failed.  d_status[i], the first that applies:
 *   BAD_TABLE     the image is invalid;
 *   BAD_ARG       src_off or out_off is not a multiple of 16;
 *   EMPTY         src_len 0;
 *   TOO_SHORT     src_len 1 at nstates 2 (at nstates 1 one byte is valid:
 *                 the seed, finish and the marker);
 *   UNSUPPORTED   src_len above 65,536: a lane's serial chain would run for
 *                 milliseconds; long messages belong on fsehip_compress_streams;
 *   SYMBOL_NOT_IN_TABLE  a byte whose count is 0 or that lies at or past
 *                 table_len (the crate indexes unchecked there, fse.rs:231-238);
 *   DST_TOO_SMALL exactly when the payload exceeds out_cap.
 * Asynchronous on `stream`; no workspace.  n_msgs == 0 returns FSE_OK and does
 * nothing; a null pointer, nstates > 2 (0 = 2) or a misaligned base is
 * BAD_ARG, n_msgs > 2^24 UNSUPPORTED, before any device use; otherwise
 * NO_DEVICE or HIP. */
int fsehip_compress_shared(uint32_t nstates, const uint8_t* d_table, const uint8_t* d_src,
                           const fsehip_stream_desc* d_desc, uint32_t n_msgs, uint8_t* d_out, uint32_t* d_comp_len,
                           uint32_t* d_payload_bits, int32_t* d_status, fsehip_stream_t stream);

/* Decode n_msgs payloads against the image d_table, one lane per message.
 * Payload i is the src_len bytes at d_in + src_off; its bytes go to d_out +
 * out_off, at most out_cap; d_out_len[i] = bytes decoded (0 for a message
 * that failed).  d_raw_len (may be NULL) gives each message's raw length:
 * then the crate's loop runs with that limit, a single-symbol table decodes,
 * and a payload that does not end with that many bytes is LENGTH_MISMATCH
 * (the block decoders stop at the raw length whatever follows; here the
 * payload must end there too: no bit left, and no step of the encoder undone
 * beyond it.  Only steps that cost no bit -- a symbol above half the table --
 * cannot be told from the end); without it the loop ends where the crate's
 * does, within out_cap.  d_status[i], the first that
 * applies: BAD_TABLE, BAD_ARG (as above), EMPTY (src_len 0), NO_MARKER (a zero
 * last byte), DST_TOO_SMALL (a raw length above out_cap), LENGTH_MISMATCH (a
 * raw length below 2 at nstates 2), SINGLE_SYMBOL (no lengths and a table of
 * one symbol: the crate would decode forever), TOO_SHORT (no room for the
 * states), then what the loop finds: LENGTH_MISMATCH with lengths,
 * DST_TOO_SMALL without.
 * Reads: no byte outside the payload (whole dwords from its end downwards, a
 * last partial dword bytewise).  Stores: 16-byte groups inside the region, the
 * last partial group bytewise, never beyond the bytes decoded.  A corrupted
 * payload ends in a status or in wrong bytes inside its region.  Call-level
 * checks and alignment as fsehip_compress_shared. */
int fsehip_decompress_shared(uint32_t nstates, const uint8_t* d_table, const uint8_t* d_in,
                             const fsehip_stream_desc* d_desc, uint32_t n_msgs, uint8_t* d_out,
                             const uint32_t* d_raw_len, uint32_t* d_out_len, int32_t* d_status,
                             fsehip_stream_t stream);

/* The bitstream as device passes over `count` fields (a prefix scan of the
 * widths places every field; HBM-bound).
 *  fsehip_bitstack_write: fields LSB-first from bit 0 of d_out; d_out must
 *    hold 4 * ceil(total / 32) bytes (<= 4 * count) and be 4-byte aligned;
 *    *d_total_bits = the bit count.
 *  fsehip_bitstack_read / fsehip_bitstream_read: d_in readable up to
 *    roundup(n_bytes, 4); d_result[0] = reads that succeed, [1] = 1 when
 *    they consume every available bit, [2] = status (NO_MARKER for a stack
 *    without its marker). */
int fsehip_bitstack_write(const uint32_t* d_vals, const uint8_t* d_nbits, uint64_t count, uint8_t* d_out,
                          uint64_t out_cap, uint64_t* d_total_bits, fsehip_stream_t stream);
int fsehip_bitstack_read(const uint8_t* d_in, uint64_t n_bytes, const uint8_t* d_nbits, uint64_t count,
                         uint32_t* d_vals, uint64_t* d_result, fsehip_stream_t stream);
int fsehip_bitstream_read(const uint8_t* d_in, uint64_t n_bytes, uint64_t total_bits, const uint8_t* d_nbits,
                          uint64_t count, uint32_t* d_vals, uint64_t* d_result, fsehip_stream_t stream);
/* The same with per-field ops (FSE_BITS_READ / PEEK / ADVANCE, device
 * pointer; NULL = all reads). */
int fsehip_bitstream_read_ops(const uint8_t* d_in, uint64_t n_bytes, uint64_t total_bits, const uint8_t* d_nbits,
                              const uint8_t* d_ops, uint64_t count, uint32_t* d_vals, uint64_t* d_result,
                              fsehip_stream_t stream);

/* histogram::count per block of block_size bytes (0 = 65536; a multiple of
 * 16 when there is more than one block, BAD_ARG otherwise; the last block
 * may be short): d_counts[b*256 + s], and d_table_len[b] = 1 + the largest
 * symbol of block b (d_table_len may be NULL).  n_total == 0 counts one
 * empty block: 256 zeros, table_len 1. */
int fsehip_histogram_blocks(const uint8_t* d_src, uint64_t n_total, uint32_t block_size, uint32_t* d_counts,
                            uint32_t* d_table_len, fsehip_stream_t stream);

/* Synthetic input (bench/tests): kind 0 = LUT generator of
 * benches/fse_benchmark.rs:5-20 with probability prob, 1 = geometric p=0.5,
 * 2 = uniform 0..239; counter-based splitmix64 (see oracle fo_generate). */
int fsehip_generate(int kind, double prob, uint64_t seed, uint32_t block_size, uint8_t* d_out,
                    uint64_t n_total, fsehip_stream_t stream);

/* Self-check of the table builds.  Every stateTable and decode table ranks its
 * positions with one LDS atomic per 64 positions (fse.rs:157-162, 329-337
 * order), which relies on an undocumented lane order of same-address LDS
 * atomics, so every table checks its ranks and is rebuilt with lane-matching
 * ranks when the check fails.  counts[0..2] = the rebuilds so far on `device`
 * by the batch encoder, the decode-table builds and the building-block table
 * calls with the shared-table images (0 on a correct GPU); reset != 0 zeroes
 * them after reading.
 * Synchronous. */
int fsehip_rank_fallbacks(int device, uint32_t counts[3], int reset);

/* Device count visible to this process (0 when HIP is unusable). */
int fsehip_device_count(void);
/* Library build identifier. */
const char* fsehip_version(void);

#ifdef __cplusplus
}
#endif
#endif
