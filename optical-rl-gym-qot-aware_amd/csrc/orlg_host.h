// orlg_host.h -- host-side helpers shared by the translation units of liborlg.so (orlg_api.hip, orlg_phy_api.hip,
// orlg_osnr.hip) and the declarations of the per-shape kernel instantiation units (orlg_inst_*.hip, one object per word
// count W so that the library builds in parallel: build.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orlg.h"
#include "orlg_device.h"

// ---------------------------------------------------------------------------------------- errors
// thread-local message of the last failure (orlg_last_error); defined in orlg_api.hip
int orlg_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#define fail orlg_fail
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(ORLG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// CPython _randommodule.c: random.Random(n) -> init_by_array(32-bit little-endian chunks of abs(n))
void orlg_mt_seed(uint32_t *mt, uint64_t seed);
int orlg_is_device_ptr(const void *ptr);
void *orlg_device_alias(const void *ptr);

// checkpoint / resume: the whole simulation state of a handle is a handful of flat device arrays
struct OrlgStatePart { void *ptr; size_t bytes; };
int orlg_state_copy(const std::vector<OrlgStatePart> &parts, void *buffer, bool save, int device, hipStream_t stream);

// Sticky error word of a handle in mapped host memory: a kernel that loses a release (queue overflow) stores 1 there, every
// entry point that waits for the stream looks at it afterwards and reports ORLG_ERR_QUEUE_FULL -- no extra copy, no extra wait.
struct OrlgErrWord {
    volatile int32_t *host;
    int32_t *dev;
};
int orlg_err_word_create(OrlgErrWord *w);
void orlg_err_word_destroy(OrlgErrWord *w);

// ---------------------------------------------------------------------------------------- per-environment traffic
// What a handle keeps of an orlg_traffic (include/orlg.h): the host arrays for the read-back, the device table of rate pairs
// the kernels read and the device group index of the grouped reduction.  A handle without traffic has empty arrays, null
// pointers and one group.
struct OrlgTrafficState {
    std::vector<double> arrival, holding;
    std::vector<int32_t> group;
    int num_groups = 1;
    OrlgRates *d_rates = nullptr;
    int32_t *d_group = nullptr;
    int64_t *d_grouped = nullptr;   // [num_groups][16] result of the grouped reduction, then its overflow word
};
// checks tr (finite positive rates, groups in range) and copies it; *arrival / *holding leave as the pair of the LARGEST offered
// load arrival_lambda[i] / holding_lambda[i] of the batch: what the handle's capacities are sized from
int orlg_traffic_check(OrlgTrafficState *ts, const orlg_traffic *tr, int batch, double *arrival, double *holding);
// device copies (call with the handle's device current); the buffers are pushed to bufs, which the handle frees
int orlg_traffic_upload(OrlgTrafficState *ts, int batch, std::vector<void *> *bufs);
int orlg_traffic_get(const OrlgTrafficState *ts, int batch, double arrival_lambda, double holding_lambda, double *arrival,
                     double *holding, int32_t *group);

// ---------------------------------------------------------------------------------------- request traces
// What a handle keeps of an orlg_trace (include/orlg.h): the device copy in the ring's layout, the length and the position
// (requests drawn so far -- every environment draws one per step, so the host knows it), and what the capacities are sized from.
struct OrlgTraceState {
    int64_t length = 0;           // requests per environment, 0 = the handle generates its traffic
    int64_t position = 0;         // requests drawn so far
    int peak = 0;                 // most requests simultaneously inside [arrival, arrival + holding], over all environments
    int pair_peak = 0;            // ... of one ordered node pair
    double mean_holding = 0.0;
    std::vector<uint32_t> req;    // host, until the upload: src | dst << 8 | rate index << 16
    double *d_arrival = nullptr, *d_holding = nullptr;
    uint32_t *d_req = nullptr;
    int64_t *d_tail = nullptr;    // (position, length): the trace handle's part of a saved state
};
// checks every entry of tr (the rules of include/orlg.h; bit_rates: the config's table, cont: lower .. higher one apart), packs the
// requests and sweeps the trace for the peaks.  Groups, if any, go to ts.
int orlg_trace_check(OrlgTraceState *st, OrlgTrafficState *ts, const orlg_trace *tr, int batch, int N, int NBR,
                     const int32_t *bit_rates, bool cont);
// device copies (the handle's device current); buffers are pushed to bufs, which the handle frees
int orlg_trace_upload(OrlgTraceState *st, const orlg_trace *tr, int batch, std::vector<void *> *bufs);
// a launch of n_steps more draws: ORLG_ERR_INVALID when it would leave the trace
int orlg_trace_admit(const OrlgTraceState *st, int n_steps);
// the position part of a saved state: written to d_tail before a save, read back and checked after a load
int orlg_trace_tail_store(OrlgTraceState *st, hipStream_t stream);
int orlg_trace_tail_load(OrlgTraceState *st, hipStream_t stream);
// the same check on a snapshot that has not been loaded yet (tail: where the 16 bytes lie in the caller's buffer, host or device)
int orlg_trace_tail_check(const OrlgTraceState *st, const void *tail);

// orlg_reduce_counters per group.  Grid-stride over the environments; every workgroup sums into a [num_groups][12] table in LDS
// (64-bit LDS atomics; at most 256 x 12 x 8 = 24 KB) and then adds its non-zero entries to out[num_groups][16], zeroed on the
// stream before, with global atomics whose result nobody reads.  Integers only, so the order of the additions does not show.
// Entries 0..9 as orlg_reduce_counters_kernel, 10 / 11 the squares of the blocked services (all-time / episode).
// Scal: OrlgEnvScalars or OrlgPhyScalars (c[8], episodes_done, q_overflow).
#define ORLG_GROUP_COLS 12
template <typename Scal>
__global__ __launch_bounds__(256) void orlg_reduce_grouped_kernel(const Scal *scal, const int32_t *group, int B, int G,
                                                                  unsigned long long *out, int *overflow) {
    extern __shared__ unsigned long long orlg_group_tab[];
    for (int i = threadIdx.x; i < G * ORLG_GROUP_COLS; i += 256) orlg_group_tab[i] = 0ull;
    __syncthreads();
    int any = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)B; i += (size_t)gridDim.x * 256) {
        int g = group ? group[i] : 0;
        if (g < 0 || g >= G) g = 0;   // (checked at create time; a table of the wrong handle must not leave the LDS table)
        unsigned long long *row = orlg_group_tab + g * ORLG_GROUP_COLS;
        const Scal &s = scal[i];
        for (int q = 0; q < 8; ++q) atomicAdd(row + q, (unsigned long long)s.c[q]);
        atomicAdd(row + 8, (unsigned long long)s.episodes_done);
        atomicAdd(row + 9, 1ull);
        const long long blocked = s.c[0] - s.c[1], eblocked = s.c[2] - s.c[3];
        atomicAdd(row + 10, (unsigned long long)(blocked * blocked));
        atomicAdd(row + 11, (unsigned long long)(eblocked * eblocked));
        any |= s.q_overflow;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < G * ORLG_GROUP_COLS; i += 256) {
        const unsigned long long v = orlg_group_tab[i];
        if (v) atomicAdd(out + (i / ORLG_GROUP_COLS) * 16 + i % ORLG_GROUP_COLS, v);
    }
    if (any) atomicOr(overflow, 1);
}
// zeroes ts->d_grouped, launches the kernel above and copies [num_groups][16] to out (host or device); *overflow = an environment
// of the batch has its overflow word set
template <typename Scal>
static int orlg_reduce_grouped(OrlgTrafficState *ts, std::vector<void *> *bufs, const Scal *scal, int B, int num_cu,
                               hipStream_t stream, int64_t *out, int *overflow) {
    const int G = ts->num_groups;
    const size_t bytes = (size_t)G * 16 * 8;
    if (!ts->d_grouped) {
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ts->d_grouped), bytes + 16));
        bufs->push_back(ts->d_grouped);
    }
    HIP_TRY(hipMemsetAsync(ts->d_grouped, 0, bytes + 16, stream));
    int nblocks = (B + 255) / 256;
    const int cap = 4 * (num_cu > 0 ? num_cu : 256);
    if (nblocks > cap) nblocks = cap;
    int *d_flag = reinterpret_cast<int *>(ts->d_grouped + (size_t)G * 16);
    hipLaunchKernelGGL(orlg_reduce_grouped_kernel<Scal>, dim3(nblocks), dim3(256), (size_t)G * ORLG_GROUP_COLS * 8, stream, scal,
                       ts->d_group, B, G, reinterpret_cast<unsigned long long *>(ts->d_grouped), d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(overflow, d_flag, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out, ts->d_grouped, bytes, hipMemcpyDefault, stream));
    return ORLG_OK;
}

// ---------------------------------------------------------------------------------------- kernel instantiation units
// Every unit exports one lookup per word count W; a W the library was not built for resolves to a null (weak) symbol.
typedef void (*orlg_rmsa_kernel_t)(const OrlgParams);
typedef void (*orlg_masks_kernel_t)(const OrlgParams, int, int, int, uint64_t *, int32_t *);
enum { ORLG_KIND_STEP = 0, ORLG_KIND_STEP_FF = 1, ORLG_KIND_RESET = 2, ORLG_KIND_GROUP = 4,
       ORLG_KIND_STEP_DF = 5, ORLG_KIND_STEP_FF_DF = 6 };   // _DF: full statistics with the links' float64 part deferred (link_replay)
#define ORLG_FOR_EACH_W(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8)
typedef void (*orlg_obs_kernel_t)(const OrlgParams, uint8_t *, int);                      // orlg_deeprmsa_obs_kernel
typedef void (*orlg_action_masks_kernel_t)(const OrlgParams, uint8_t *, int, uint64_t *);   // orlg_action_masks_kernel
#define ORLG_DECL_W(n)                                                                           \
    orlg_rmsa_kernel_t orlg_wave_kernel_W##n(int kind, int stats) __attribute__((weak));          \
    orlg_masks_kernel_t orlg_masks_kernel_W##n() __attribute__((weak));                           \
    orlg_obs_kernel_t orlg_obs_kernel_W##n() __attribute__((weak));                               \
    orlg_action_masks_kernel_t orlg_action_masks_kernel_W##n() __attribute__((weak));             \
    orlg_rmsa_kernel_t orlg_group_kernel_W##n(int stats) __attribute__((weak));
ORLG_FOR_EACH_W(ORLG_DECL_W)
#undef ORLG_DECL_W

struct OrlgPhyParams;
typedef void (*orlg_phy_kernel_t)(const OrlgPhyParams);
#define ORLG_FOR_EACH_PHY_W(X) X(1) X(2) X(3) X(4) X(5)
#define ORLG_DECL_PHY_W(n)                                                          \
    orlg_phy_kernel_t orlg_phy_kernel_W##n(int variant) __attribute__((weak));      \
    orlg_phy_kernel_t orlg_phy_trace_kernel_W##n(int variant) __attribute__((weak));   /* orlg_inst_phy_trace.hip */
ORLG_FOR_EACH_PHY_W(ORLG_DECL_PHY_W)
#undef ORLG_DECL_PHY_W
