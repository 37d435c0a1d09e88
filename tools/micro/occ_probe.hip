// LDS allocation granule and real residency probe (diagnostics, not product
// code): how many workgroups a CU holds at once for a given LDS size.
//
// A launch of far more workgroups than can be resident, each with D bytes of
// dynamic LDS.  A workgroup notes the real-time counter (100 MHz) when it
// starts, waits T = 100 us on that counter (no memory polling, a hard
// iteration cap) and exits.  The workgroups that start within T/2 of the
// first are the ones the device held at once: their number over the CU count
// is W, the resident workgroups per CU at D.  The launch time, ceil(G / (CUs
// x W)) x T, is printed as a cross-check.  W against D steps down where D
// crosses a multiple of the allocation granule, which fixes the granule.
//
//   occ_probe [LIB]    LIB: a libfsehip*.so; its fsehipx_occupancy report (what
//                      hipOccupancyMaxActiveBlocksPerMultiprocessor says for the
//                      encode kernels) is printed beside the measurement
//
// Sweeps: one-wave workgroups at D = 12,288 .. 15,360 B in 256 B steps (the
// encoder's range), and 512-thread workgroups at the decoder's 53,296 and
// 54,324 B (3 against 2 per CU in round 5).
// Build: hipcc -O3 --offload-arch=gfx950 occ_probe.hip -o occ_probe -ldl
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

constexpr uint64_t HOLD_TICKS = 10000;  // 100 us of the 100 MHz real-time counter
constexpr uint32_t ITER_CAP = 1u << 14;  // ~0.3 us per iteration: the wait ends within ~5 ms whatever the counter does

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            printf("%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);        \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

extern __shared__ uint32_t dyn_lds[];

template <int THREADS>
__global__ __launch_bounds__(THREADS) void hold_kernel(uint64_t* start, uint32_t n, uint32_t touch) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0 && blockIdx.x < n) start[blockIdx.x] = t0;
    if (touch) dyn_lds[threadIdx.x] = touch;  // never taken: keeps the dynamic segment referenced
    for (uint32_t it = 0; it < ITER_CAP; ++it) {
        if (__builtin_amdgcn_s_memrealtime() - t0 >= HOLD_TICKS) break;
        __builtin_amdgcn_s_sleep(8);
    }
}

template <int THREADS>
int measure(uint32_t lds, int cus, uint32_t per_cu, uint64_t* d_start) {
    const uint32_t grid = (uint32_t)cus * per_cu;
    int api = -1;
    CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&api, hold_kernel<THREADS>, THREADS, lds));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    float ms = 0;
    std::vector<uint64_t> h(grid);
    for (int rep = 0; rep < 2; ++rep) {  // the second launch is the measurement (the first loads the code object)
        CHECK(hipEventRecord(a));
        hipLaunchKernelGGL(hold_kernel<THREADS>, dim3(grid), dim3(THREADS), lds, 0, d_start, grid, 0u);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        CHECK(hipEventElapsedTime(&ms, a, b));
    }
    CHECK(hipMemcpy(h.data(), d_start, grid * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const uint64_t first = *std::min_element(h.begin(), h.end());
    uint32_t at_once = 0;
    for (uint64_t t : h) at_once += (t - first < HOLD_TICKS / 2) ? 1u : 0u;
    printf("threads %3d  lds %6u B  resident %5u = %6.2f per CU  launch %.3f ms = %.2f T  (occupancy API: %d)\n", THREADS,
           lds, at_once, (double)at_once / cus, ms, ms / (HOLD_TICKS / 100000.0), api);
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
    return 0;
}

int main(int argc, char** argv) {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    printf("%s: %d CUs, %zu B LDS per workgroup max\n", prop.gcnArchName, cus, prop.sharedMemPerBlock);
    if (argc > 1) {
        void* lib = dlopen(argv[1], RTLD_NOW);
        auto occ = lib ? reinterpret_cast<int (*)(char*, int)>(dlsym(lib, "fsehipx_occupancy")) : nullptr;
        if (occ) {
            static char buf[4096];
            const int n = occ(buf, (int)sizeof buf - 1);
            printf("%s:\n%.*s", argv[1], n, buf);
        } else {
            printf("%s: no fsehipx_occupancy (%s)\n", argv[1], lib ? "symbol missing" : dlerror());
        }
    }
    constexpr uint32_t PER_CU_1W = 40, PER_CU_8W = 8;  // more than the 32 waves a CU holds
    uint64_t* d_start = nullptr;
    CHECK(hipMalloc(&d_start, (size_t)cus * PER_CU_1W * sizeof(uint64_t)));
    for (uint32_t lds = 12288; lds <= 15360; lds += 256)
        if (measure<64>(lds, cus, PER_CU_1W, d_start)) return 1;
    // the encoder's sizes: the parent's 14,768 B static + 62 B pad, its static size alone, the overlaid layout
    for (uint32_t lds : {14830u, 14768u, 12592u})
        if (measure<64>(lds, cus, PER_CU_1W, d_start)) return 1;
    for (uint32_t lds : {53296u, 54324u})
        if (measure<512>(lds, cus, PER_CU_8W, d_start)) return 1;
    CHECK(hipFree(d_start));
    return 0;
}
