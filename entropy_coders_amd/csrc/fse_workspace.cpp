// fse_workspace.cpp -- the stream workspaces, the host calls' staging
// (fse_workspace.h) and the diagnostics build's stamps report.
#include <stdio.h>

#include <atomic>
#include <memory>
#include <vector>

#include "fse_capi_common.h"

namespace fsehip {
namespace capi {

namespace {
std::mutex g_ws_mu;
std::vector<std::unique_ptr<Workspace>> g_ws;
}  // namespace

thread_local StageBufs<false, STAGE_KINDS> g_stage;
thread_local StageBufs<true, PIN_KINDS> g_pin;

bool device_ok() {
    static std::atomic<bool> seen{false};  // devices do not go away: ask the runtime once (~17 us a call)
    if (seen.load(std::memory_order_relaxed)) return true;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return false;
    seen.store(true, std::memory_order_relaxed);
    return true;
}

Lease::Lease(void* stream) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    {
        std::lock_guard<std::mutex> g(g_ws_mu);
        for (auto& x : g_ws)
            if (x->dev == dev && x->stream == stream) ws = x.get();
        if (!ws) {
            g_ws.push_back(std::make_unique<Workspace>());
            ws = g_ws.back().get();
            ws->dev = dev;
            ws->stream = stream;
        }
    }
    lk = std::unique_lock<std::mutex>(ws->mu);
}

void* Lease::get(int tag, uint64_t bytes, bool optional) {
    if (!ws) return nullptr;
    if (ws->bytes[tag] < bytes) {
        if (optional && ws->failed[tag] && bytes >= ws->failed[tag]) return nullptr;
        if (ws->ptr[tag]) {
            (void)hipStreamSynchronize(static_cast<hipStream_t>(ws->stream));
            (void)hipFree(ws->ptr[tag]);
            ws->ptr[tag] = nullptr;
        }
        ws->bytes[tag] = 0;
        if (hipMalloc(&ws->ptr[tag], bytes) != hipSuccess) {
            (void)hipGetLastError();  // an optional buffer's failure must not surface in a later launch check
            ws->ptr[tag] = nullptr;
            if (optional) ws->failed[tag] = ws->failed[tag] ? std::min(ws->failed[tag], bytes) : bytes;
            return nullptr;
        }
        ws->bytes[tag] = bytes;
    }
    return ws->ptr[tag];
}

PinBuf* Lease::pin_get(uint64_t bytes) {
    if (!ws) return nullptr;
    // among the free buffers: one that holds `bytes`, else one never
    // allocated, else one to regrow.  hipHostFree waits for every stream
    // of the device, so a regrow makes the call wait for the work queued
    // before it, as a workspace buffer's growth does.
    PinBuf* pick = nullptr;
    int best = -1;
    for (PinBuf& b : ws->pin) {
        if (b.busy && hipEventQuery(b.ev) == hipSuccess) b.busy = false;
        (void)hipGetLastError();  // hipErrorNotReady is no error
        if (b.busy) continue;
        const int rank = b.cap >= bytes ? 2 : !b.p ? 1 : 0;
        if (rank > best) {
            best = rank;
            pick = &b;
        }
    }
    if (!pick) {
        pick = &ws->pin[ws->pin_next];
        ws->pin_next = (ws->pin_next + 1) % kPinBufs;
        if (hipEventSynchronize(pick->ev) != hipSuccess) return nullptr;
        pick->busy = false;
    }
    if (pick->cap < bytes) {
        if (pick->p) (void)hipHostFree(pick->p);
        pick->p = nullptr;
        pick->cap = 0;
        // powers of two from kPinMin: lists of a few thousand ranges never regrow a buffer
        uint64_t want = kPinMin;
        while (want < bytes) want <<= 1;
        if (hipHostMalloc(&pick->p, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            pick->p = nullptr;
            return nullptr;
        }
        pick->cap = want;
    }
    if (!pick->ev && hipEventCreateWithFlags(&pick->ev, hipEventDisableTiming) != hipSuccess) return nullptr;
    return pick;
}

bool Lease::pin_sent(PinBuf* b) {
    if (hipEventRecord(b->ev, static_cast<hipStream_t>(ws->stream)) != hipSuccess) {
        // the copy's end is unknown: wait for it here rather than hand the buffer out early
        (void)hipStreamSynchronize(static_cast<hipStream_t>(ws->stream));
        return false;
    }
    b->busy = true;
    return true;
}

int release_workspaces(int device, void* stream, bool any_stream) {
    std::vector<Workspace*> hit;
    {
        std::lock_guard<std::mutex> g(g_ws_mu);
        for (auto& x : g_ws)
            if ((device < 0 || x->dev == device) && (any_stream || x->stream == stream)) hit.push_back(x.get());
    }
    int prev = 0;
    (void)hipGetDevice(&prev);
    int rc = FSE_OK;
    for (Workspace* w : hit) {
        std::lock_guard<std::mutex> lk(w->mu);
        if (hipSetDevice(w->dev) != hipSuccess) {
            (void)hipGetLastError();
            rc = FSE_ERR_HIP;
            continue;
        }
        bool any = false;
        for (int t = 0; t < SCRATCH_KINDS; ++t) any = any || w->ptr[t];
        for (const PinBuf& b : w->pin) any = any || b.p;
        if (any && hipStreamSynchronize(static_cast<hipStream_t>(w->stream)) != hipSuccess) rc = FSE_ERR_HIP;
        for (int t = 0; t < SCRATCH_KINDS; ++t) {
            if (w->ptr[t] && hipFree(w->ptr[t]) != hipSuccess) rc = FSE_ERR_HIP;
            w->ptr[t] = nullptr;
            w->bytes[t] = 0;
            w->failed[t] = 0;
        }
        for (PinBuf& b : w->pin) {
            if (b.p && hipHostFree(b.p) != hipSuccess) rc = FSE_ERR_HIP;
            if (b.ev) (void)hipEventDestroy(b.ev);
            b = PinBuf();
        }
        w->pin_next = 0;
    }
    (void)hipSetDevice(prev);
    return rc;
}

// ------------------------------------------------------- stamps report

Stamps g_stamps_enc, g_stamps_dec, g_stamps_dt;

uint64_t* Stamps::get(size_t groups) {
    if (!env_u32("FSEHIP_STAMPS", 0)) return nullptr;
    size_t need = groups * fsehip::kStamps;
    if (n < need) {
        if (d) (void)hipFree(d);
        if (hipMalloc(&d, need * 8) != hipSuccess) return d = nullptr;
        n = need;
    }
    (void)hipMemset(d, 0, need * 8);
    return d;
}

void Stamps::report(const char* what, size_t groups, hipStream_t s) {
    if (!d) return;
    (void)hipStreamSynchronize(s);
    std::vector<uint64_t> h(groups * fsehip::kStamps);
    (void)hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost);
    // deltas between consecutive recorded slots (kernels may skip slots);
    // per XCD (workgroups are placed round-robin over the 8 XCDs) the
    // span from the first start to the last stamp, for the mean number
    // of workgroups in flight per CU (32 CUs per XCD)
    double acc[fsehip::kStamps] = {0}, life = 0;
    size_t cnt[fsehip::kStamps] = {0}, nlife = 0;
    uint64_t lo_x[8], hi_x[8];
    for (int x = 0; x < 8; ++x) lo_x[x] = ~0ull, hi_x[x] = 0;
    for (size_t g = 0; g < groups; ++g) {
        const uint64_t* r = &h[g * fsehip::kStamps];
        int prev = -1;
        for (int k = 0; k < fsehip::kStamps - 1; ++k) {
            if (!r[k]) continue;
            if (prev >= 0 && r[k] >= r[prev]) { acc[k] += (double)(r[k] - r[prev]); cnt[k]++; }
            prev = k;
        }
        if (r[0] && prev > 0 && r[prev] >= r[0]) {
            life += (double)(r[prev] - r[0]);
            nlife++;
            lo_x[g % 8] = std::min(lo_x[g % 8], r[0]);
            hi_x[g % 8] = std::max(hi_x[g % 8], r[prev]);
        }
    }
    fprintf(stderr, "[stamps] %s:", what);
    for (int k = 1; k < fsehip::kStamps - 1; ++k)
        if (cnt[k]) fprintf(stderr, " %d:%.0f", k, acc[k] / cnt[k]);
    double span = 0;
    for (int x = 0; x < 8; ++x)
        if (hi_x[x] > lo_x[x]) span += (double)(hi_x[x] - lo_x[x]);
    fprintf(stderr, " (mean cycles per workgroup since the previous stamp)\n");
    if (nlife && span > 0)
        fprintf(stderr, "[stamps] %s: lifetime %.0f cycles, XCD span %.0f cycles, %.2f workgroups in flight per CU\n",
                what, life / nlife, span / 8, life / (span * 32.0) * ((double)groups / nlife));
    // slot kStamps-1: kernel-defined counters (low / high 32 bits), averaged
    double lo = 0, hi = 0;
    for (size_t g = 0; g < groups; ++g) {
        const uint64_t v = h[g * fsehip::kStamps + fsehip::kStamps - 1];
        lo += (double)(v & 0xFFFFFFFFu);
        hi += (double)(v >> 32);
    }
    fprintf(stderr, "[stamps] %s counters: lo %.3f hi %.3f (mean per workgroup)\n", what, lo / groups, hi / groups);
}

}  // namespace capi
}  // namespace fsehip
