// fse_workspace.h -- memory the C ABI calls work in: the per-(device, stream)
// device workspace with its pinned list buffers, and the per-thread staging of
// the host-pointer calls.  Internal (hidden) to libfsehip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>

namespace fsehip {
namespace capi __attribute__((visibility("hidden"))) {

inline uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

bool device_ok();  // a HIP device exists (asked of the runtime once)

// Per-(device, stream) grow-only device workspace for the two-kernel encode
// and decode.  A caller holds the workspace's lock (a Lease) from taking the
// buffers until its last launch on them is enqueued: calls on one stream then
// use the buffers in stream order, and a call that has to grow a buffer
// synchronises the stream (the work of earlier holders has been enqueued on
// it) before freeing the old one.  Different streams get different
// workspaces.
enum {
    SCRATCH_DT = 0,
    SCRATCH_DTINFO = 1,
    SCRATCH_BITS = 2,
    SCRATCH_STATES = 3,
    SCRATCH_BULK = 4,
    SCRATCH_HDR = 5,  // the lane-parallel header parse's output (optional)
    SCRATCH_SPREAD = 6,  // the L >= 13 encoder's spread symbols when the slots cannot hold them
    // the frame calls, per chunk of blocks (fsehip.h workspace note)
    SCRATCH_FRAME_SLOTS = 7,  // the chunk's slots
    SCRATCH_FRAME_META = 8,   // checkpoints, comp_len, status, record type
    SCRATCH_FRAME_SCAN = 9,   // record offsets + the running frame offset
    // fsehip_frame_decompress_ranges
    SCRATCH_FRAME_LIST = 10,    // the planner's lists and the per-listed-block results
    SCRATCH_FRAME_BOUNCE = 11,  // a bounce chunk's decoded blocks
    SCRATCH_KINDS = 12
};
// Pinned host staging for lists an asynchronous call uploads (the range
// planner's).  A buffer is busy until the event recorded after its copy has
// passed; a call takes a free one or adds one, so it never waits for the
// stream.  At most kPinBufs per workspace: beyond that the oldest is waited for.
constexpr int kPinBufs = 8;
constexpr uint64_t kPinMin = 64u << 10;  // smallest capacity of one
struct PinBuf {
    void* p = nullptr;
    uint64_t cap = 0;
    hipEvent_t ev = nullptr;
    bool busy = false;
};
struct Workspace {
    int dev;
    void* stream;
    std::mutex mu;
    void* ptr[SCRATCH_KINDS] = {};
    uint64_t bytes[SCRATCH_KINDS] = {};
    // smallest size whose allocation failed (optional buffers only): later
    // calls asking for as much or more take their fallback at once instead of
    // retrying a multi-GiB hipMalloc on every call; cleared by
    // fsehip_release_workspace
    uint64_t failed[SCRATCH_KINDS] = {};
    PinBuf pin[kPinBufs];
    int pin_next = 0;  // the oldest busy buffer when all are busy
};

struct Lease {
    Workspace* ws = nullptr;
    std::unique_lock<std::mutex> lk;
    explicit Lease(void* stream);
    // `optional`: the caller has a fallback without the buffer (the
    // deferred-symbol decode), so a failed size is remembered
    void* get(int tag, uint64_t bytes, bool optional = false);
    // a pinned host buffer of `bytes` no pending copy reads; pin_sent() after its copy is enqueued
    PinBuf* pin_get(uint64_t bytes);
    bool pin_sent(PinBuf* b);
};

// Free every buffer of the matching workspaces (device < 0: all devices;
// stream is matched as given) after the work enqueued on their streams.
int release_workspaces(int device, void* stream, bool any_stream);

// Staging for the host-pointer entry points: a grow-only array of K buffers
// per thread, in device memory or (Pinned) in pinned host memory: a pageable
// hipMemcpy costs ~100 us per call here (profiles/r04/single_stream/), a copy
// through pinned memory a few.  The device buffers belong to one device:
// when the current device has changed, all are dropped.
template <bool Pinned, int K>
struct StageBufs {
    static constexpr size_t kMin = Pinned ? size_t(64) << 10 : 4096;
    static hipError_t alloc(void** p, size_t n) { return Pinned ? hipHostMalloc(p, n, hipHostMallocDefault) : hipMalloc(p, n); }
    static hipError_t free(void* p) { return Pinned ? hipHostFree(p) : hipFree(p); }
    uint8_t* buf[K] = {};
    size_t cap[K] = {};
    int device = -1;
    ~StageBufs() { release(); }
    void drop(int i) {
        if (buf[i]) (void)free(buf[i]);
        buf[i] = nullptr;
        cap[i] = 0;
    }
    void release() {
        for (int i = 0; i < K; ++i) drop(i);
    }
    uint8_t* get(int i, size_t bytes) {
        if (!Pinned) {
            int dev = 0;
            (void)hipGetDevice(&dev);
            if (dev != device) release();
            device = dev;
        }
        if (cap[i] < bytes) {
            drop(i);
            void* p = nullptr;
            const size_t want = round_up(std::max<size_t>(bytes, kMin), 4096);
            if (alloc(&p, want) != hipSuccess) return nullptr;
            buf[i] = static_cast<uint8_t*>(p);
            cap[i] = want;
        }
        return buf[i];
    }
};
// The slots.  A host call owns the slots it takes until it returns, and the
// host calls that call others do so one after the other, never with a slot of
// their own live across the call: fse_*_many runs its batches (BATCH_*) and
// then its single streams (compress_one / decompress_one: SRC, OUT, REC,
// TABLES, FTAB) in turn; fse_compress_nh runs fse_compress and then
// norm_histogram_read (REC); histogram_new is histogram_count.  The device
// calls they reach (fsehip_*) take none.  Every call that used a pinned buffer
// synchronises the null stream before it returns, errors included.
enum StageSlot {
    STAGE_SRC = 0,        // the call's input (the bit calls: values / stream)
    STAGE_OUT = 1,        // its output (the bit calls: widths)
    STAGE_REC = 2,        // a small record: Meta, counts, a norm histogram's I/O, a total, a result triple
    STAGE_TABLES = 3,     // decompress_one's decode table (the bit calls: ops)
    STAGE_BATCH_IN = 4,   // a batch's staged input (table_new: its histogram and table)
    STAGE_BATCH_OUT = 5,  // a batch's output regions (the bit calls: output)
    STAGE_FTAB = 6,       // decompress_one's fused bulk table
    STAGE_BATCH_RES = 7,  // compress_batch's records and packed streams
    STAGE_KINDS = 8
};
// compress_batch takes PIN_RET twice, for the records and then for the packed
// streams, whose size the records tell: the second get() may free the buffer,
// so the records are copied out in between.
enum PinSlot { PIN_IN = 0, PIN_RET = 1, PIN_KINDS = 2 };
constexpr size_t kPinOut = size_t(4) << 20;  // output bytes returned through PIN_RET; the rest by hipMemcpy
extern thread_local StageBufs<false, STAGE_KINDS> g_stage;
extern thread_local StageBufs<true, PIN_KINDS> g_pin;

}  // namespace capi
}  // namespace fsehip
