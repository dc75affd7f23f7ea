// orlg_host.h -- the host side that the translation units of liborlg.so share (orlg_host.hip defines it; the RMSA API's
// units through orlg_rmsa_host.h, orlg_phy_api.hip and orlg_osnr.hip use it): errors, the handle core of both C APIs with the functions that work on it, the
// helper kernels that differ only in the scalar record, and what a launch of a step kernel does around the launch itself.  The
// kernel instantiations, their keys and names: orlg_variants.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/orlg.h"
#include "orlg_device.h"
#include "orlg_variants.h"

// ---------------------------------------------------------------------------------------- errors
// thread-local message of the last failure (orlg_last_error)
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
// device copies (call with the handle's device current); the handle owns the buffers
struct OrlgHandle;
int orlg_traffic_upload(OrlgHandle *h, int batch);
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
// requests and sweeps the trace for the peaks.  Groups, if any, go to ts.  *arrival / *holding leave as what sizes such a handle's
// capacities next to the peaks: one request per unit of time, released after the trace's mean holding time
int orlg_trace_check(OrlgTraceState *st, OrlgTrafficState *ts, const orlg_trace *tr, int batch, int N, int NBR,
                     const int32_t *bit_rates, bool cont, double *arrival, double *holding);
// device copies (the handle's device current); the handle owns the buffers
int orlg_trace_upload(OrlgHandle *h, const orlg_trace *tr, int batch);
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
// Entries 0..9 as orlg_reduce16_kernel, 10 / 11 the squares of the blocked services (all-time / episode).
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
// ---------------------------------------------------------------------------------------- handle core
// A device buffer of the handle that is allocated on first use and replaced by a larger one when a call needs more.
struct OrlgScratch {
    void *ptr = nullptr;
    size_t cap = 0;
    unsigned char *bytes() const { return static_cast<unsigned char *>(ptr); }
};
#define ORLG_IO_SLOTS 16      // >= ORLG_NUM_OUTS, ORLG_PHY_NUM_OUTS
#define ORLG_EXTRA_SLOTS 7   // a variant's own buffers of that kind (staged actions, the float64 shares)

// What orlg_env and orlg_phy_env have in common: the device, the stream, the launch geometry of the step kernel, every device
// allocation, the sticky error word, traffic and trace.  It owns what it holds: deleting a handle waits for its stream and frees
// all of it, at whatever point of a create the handle is dropped.
struct OrlgHandle {
    int device = 0, num_cu = 0;
    int W = 0, waves_per_block = 0, num_paths = 0;
    size_t lds_block_bytes = 0;
    uint32_t ticket_base = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool opened = false;             // orlg_handle_open selected the device: there may be something to free on it
    std::vector<void *> bufs;        // allocations that live as long as the handle (orlg_handle_alloc)
    OrlgScratch staging;             // read-backs and the outputs of the observation / mask entry points
    OrlgScratch io[ORLG_IO_SLOTS];   // per-step outputs bound for pageable host memory, one per output slot
    OrlgScratch extra[ORLG_EXTRA_SLOTS];
    OrlgErrWord err = {nullptr, nullptr};   // sticky error word the kernels set on an overflow
    std::string overflow_message;    // what orlg_handle_sync_check reports then (the variant words it, with its capacities)
    char last_kernel[160] = "";       // name and shape of the kernel behind the last step / reset launch
    OrlgTrafficState traffic;        // per-environment rates and groups (*_create_traffic)
    OrlgTraceState trace;            // request trace and its position (*_create_trace)
    OrlgHandle() = default;
    OrlgHandle(const OrlgHandle &) = delete;
    OrlgHandle &operator=(const OrlgHandle &) = delete;
    ~OrlgHandle();
};
// device count and range checks (ORLG_ERR_NO_DEVICE / ORLG_ERR_INVALID), hipSetDevice, the CU count, the stream, the error word
int orlg_handle_open(OrlgHandle *h, int device);
int orlg_handle_set_stream(OrlgHandle *h, void *hip_stream);
// wait for the handle's stream, then report an overflow a kernel flagged (ORLG_ERR_QUEUE_FULL is sticky until a full reset)
int orlg_handle_sync_check(OrlgHandle *h);
int orlg_handle_last_kernel(const OrlgHandle *h, char *buf, int32_t cap);
// Around a launch.  lds: let `kernel` use `bytes` of dynamic LDS.  resident: the workgroups of `kernel` (`block` threads, `lds`
// bytes) the device holds at a time = the largest grid of a work queue, asked once and kept in *resident (0 = not asked yet).
// launched: last_kernel = `name grid= block= lds=`, then ` body=lean` or ` body=full` for the four-environments-per-wave kernel
// (orlg_rmsa_group_body) and last ` chunks=` where there are any (callers read the end of the string for it); the name is the
// key's (orlg_kernel_name).
int orlg_kernel_lds(const void *kernel, size_t bytes);
int orlg_handle_resident(OrlgHandle *h, const void *kernel, int block, size_t lds, int *resident);
void orlg_handle_note_launch(OrlgHandle *h, const char *name, int grid, int block, size_t lds, int chunks, const char *body);
template <typename Key>
static void orlg_handle_launched(OrlgHandle *h, const Key &key, int grid, int block, size_t lds, int chunks = 0, const char *body = nullptr) {
    char name[96];   // (the longest: the group kernel's nine arguments, 67 characters)
    orlg_kernel_name(name, sizeof(name), h->W, key);
    orlg_handle_note_launch(h, name, grid, block, lds, chunks, body);
}
// allocate `bytes` (16 when that is 0) and remember them in bufs; then copy `bytes` from host, or zero them, or neither
int orlg_handle_alloc_bytes(OrlgHandle *h, void **out, size_t bytes, const void *host, bool zero);
template <typename T>
static int orlg_handle_alloc(OrlgHandle *h, T **out, size_t count, bool zero = false) {
    void *ptr = nullptr;
    int rc = orlg_handle_alloc_bytes(h, &ptr, count * sizeof(T), nullptr, zero);
    *out = static_cast<T *>(ptr);
    return rc;
}
template <typename T>
static int orlg_handle_upload(OrlgHandle *h, T **out, const T *host, size_t count) {
    void *ptr = nullptr;
    int rc = orlg_handle_alloc_bytes(h, &ptr, count * sizeof(T), host, false);
    *out = static_cast<T *>(ptr);
    return rc;
}
int orlg_scratch_grow(OrlgScratch *s, size_t bytes);   // at least `bytes`; the contents do not survive a growth
static inline int orlg_handle_staging(OrlgHandle *h, size_t bytes) { return orlg_scratch_grow(&h->staging, bytes); }
// MT19937 states of a batch: seeds[i], or base_seed + i without an array; a trace handle has no generator and gets zeroes (the
// array is part of its saved state all the same).  Waits for the copy.
int orlg_seed_states(OrlgHandle *h, uint32_t *d_mt, int batch, const uint64_t *seeds, uint64_t base_seed, bool trace);
// the end of a create, after the clear and INIT launches: wait for them; the initial reset of a trace handle drew request 0
int orlg_handle_initial_wait(OrlgHandle *h);

// Per-step outputs of one launch of n_steps * B = count elements each.  place: outs[i] = where the kernel writes output i -- the
// caller's pointer when that is device memory (orlg_is_device_ptr), h->io[i] grown to fit otherwise, nullptr when not asked for;
// returns the mask of the outputs asked for.  collect: copies the staged ones to the caller (*any = there was one: the caller waits).
struct OrlgOut { void *user; size_t elem; };
int orlg_handle_place(OrlgHandle *h, const OrlgOut *slots, int n, size_t count, void **outs, int32_t *out_mask);
int orlg_handle_collect(OrlgHandle *h, const OrlgOut *slots, int n, size_t count, void *const *outs, bool *any);

// Saved state = the concatenation of `parts`; a trace handle's position travels as the part OrlgTraceState::d_tail, written before
// a save and checked inside the caller's buffer before a load copies anything.  A load leaves the error word cleared.
int64_t orlg_handle_state_size(const std::vector<OrlgStatePart> &parts);
int orlg_handle_state_save(OrlgHandle *h, const std::vector<OrlgStatePart> &parts, void *buffer);
int orlg_handle_state_load(OrlgHandle *h, const std::vector<OrlgStatePart> &parts, const void *buffer);

// The table blob every workgroup stages into LDS: put returns the byte offset (16-byte aligned) of what it appends.
struct OrlgBlob {
    std::vector<unsigned char> bytes;
    int32_t put(const void *src, size_t n) {
        const size_t at = bytes.size();
        bytes.resize((at + n + 15) & ~(size_t)15, 0);
        memcpy(bytes.data() + at, src, n);
        return (int32_t)at;
    }
};
// OrlgPathRec of every path of t from the CSR arrays; hops, CSR and link indices checked.  link_fmt words a link outside 0..E-1
// (printf arguments: path, link).  The spectral efficiency is copied unchecked.  The link bytes past a path's end are filled
// with the path's first link: the padding rule stated at OrlgPathRec (orlg_device.h), which the group kernel's policy relies on.
int orlg_path_records(const orlg_topology *t, int E, const char *link_fmt, std::vector<OrlgPathRec> *recs);

// ---------------------------------------------------------------------------------------- kernels over the scalar records
// Scal: OrlgEnvScalars or OrlgPhyScalars (c[8], episodes_done, q_overflow, mt_idx, ring_pos, ring_cnt)
template <typename Scal>
__global__ void orlg_reseed_kernel(Scal *scal, int B) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B; i += gridDim.x * blockDim.x) {
        scal[i].mt_idx = ORLG_MT_N;               // a freshly seeded generator: the first draw regenerates the state
        scal[i].ring_pos = 0; scal[i].ring_cnt = 0;   // arrivals pre-generated from the old generator are dropped
    }
}
// the sticky error word (mapped host memory: a plain store, no atomic across the bus) recomputed from the scalars
template <typename Scal>
__global__ void orlg_overflow_store_kernel(const Scal *scal, int B, int *err_flag) {
    int any = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B; i += gridDim.x * blockDim.x) any |= scal[i].q_overflow;
    if (any) *err_flag = 1;
}
// Sum of the counters of all envs (one workgroup; 64-bit integer adds, deterministic order per lane then a fixed tree): the
// vector the multi-GPU layer all-reduces.  out[16]: c[0..7], episodes done, environments; with COLS = 11 then the sum of
// q_overflow; zeroes after.
template <typename Scal, int COLS>
__global__ __launch_bounds__(256) void orlg_reduce16_kernel(const Scal *scal, int B, long long *out) {
    __shared__ long long part[256][COLS];
    long long acc[COLS];
    for (int q = 0; q < COLS; ++q) acc[q] = 0;
    for (int i = threadIdx.x; i < B; i += 256) {
        for (int q = 0; q < 8; ++q) acc[q] += scal[i].c[q];
        acc[8] += scal[i].episodes_done;
        acc[9] += 1;
        if constexpr (COLS > 10) acc[10] += scal[i].q_overflow;
    }
    for (int q = 0; q < COLS; ++q) part[threadIdx.x][q] = acc[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int q = 0; q < COLS; ++q) part[threadIdx.x][q] += part[threadIdx.x + s][q];
        __syncthreads();
    }
    if (threadIdx.x < 16) out[threadIdx.x] = threadIdx.x < COLS ? part[0][threadIdx.x] : 0;
}

// *_reseed: fresh generators between two launches; the pending requests stay
template <typename Scal>
static int orlg_handle_reseed(OrlgHandle *h, uint32_t *d_mt, Scal *scal, int B, const uint64_t *seeds, uint64_t base_seed) {
    if (!h) return fail(ORLG_ERR_INVALID, "null handle");
    if (h->trace.length > 0) return fail(ORLG_ERR_INVALID, "a handle that replays a trace has no generator to seed");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int rc = orlg_seed_states(h, d_mt, B, seeds, base_seed, false);
    if (rc) return rc;
    hipLaunchKernelGGL(orlg_reseed_kernel<Scal>, dim3(64), dim3(256), 0, h->stream, scal, B);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ORLG_OK;
}
// *_load_state: the sticky error word describes the state the handle holds, so it is recomputed from the loaded scalars (a clean
// checkpoint clears a reported ORLG_ERR_QUEUE_FULL, a checkpoint of an overflowed batch brings it back)
template <typename Scal>
static int orlg_handle_load(OrlgHandle *h, const std::vector<OrlgStatePart> &parts, const void *buffer, const Scal *scal, int B) {
    int rc = orlg_handle_state_load(h, parts, buffer);
    if (rc) return rc;
    hipLaunchKernelGGL(orlg_overflow_store_kernel<Scal>, dim3(64), dim3(256), 0, h->stream, scal, B, h->err.dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ORLG_OK;
}
// *_reduce_counters_grouped up to the wait: zeroes traffic.d_grouped, launches orlg_reduce_grouped_kernel and queues the copies of
// [num_groups][16] to out (host or device) and of the batch's overflow word to *overflow (host)
template <typename Scal>
static int orlg_reduce_grouped(OrlgHandle *h, const Scal *scal, int B, int64_t *out, int *overflow) {
    OrlgTrafficState *ts = &h->traffic;
    const int G = ts->num_groups;
    const size_t bytes = (size_t)G * 16 * 8;
    if (!ts->d_grouped) {
        int rc = orlg_handle_alloc(h, &ts->d_grouped, (bytes + 16) / 8);
        if (rc) return rc;
    }
    HIP_TRY(hipMemsetAsync(ts->d_grouped, 0, bytes + 16, h->stream));
    int nblocks = (B + 255) / 256;
    if (nblocks > 4 * h->num_cu) nblocks = 4 * h->num_cu;
    int *d_flag = reinterpret_cast<int *>(ts->d_grouped + (size_t)G * 16);
    hipLaunchKernelGGL(orlg_reduce_grouped_kernel<Scal>, dim3(nblocks), dim3(256), (size_t)G * ORLG_GROUP_COLS * 8, h->stream, scal,
                       ts->d_group, B, G, reinterpret_cast<unsigned long long *>(ts->d_grouped), d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(overflow, d_flag, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(out, ts->d_grouped, bytes, hipMemcpyDefault, h->stream));
    return ORLG_OK;
}
