// orlg_host.hip -- the host side both C APIs share (orlg_host.h): the library's error message, pointer classification, MT19937
// seeding, per-environment traffic, request traces and the handle core with the functions that work on it.  No kernels.
#include "orlg_host.h"

// ---------------------------------------------------------------------------------------- errors
static thread_local std::string g_err;
int orlg_fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int orlg_err_word_create(OrlgErrWord *w) {
    void *h = nullptr, *d = nullptr;
    w->host = nullptr; w->dev = nullptr;
    HIP_TRY(hipHostMalloc(&h, 64, hipHostMallocMapped));
    memset(h, 0, 64);
    hipError_t er = hipHostGetDevicePointer(&d, h, 0);
    if (er != hipSuccess) { (void)hipHostFree(h); return fail(ORLG_ERR_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(er)); }
    w->host = static_cast<volatile int32_t *>(h);
    w->dev = static_cast<int32_t *>(d);
    return ORLG_OK;
}
void orlg_err_word_destroy(OrlgErrWord *w) {
    if (w->host) (void)hipHostFree(const_cast<int32_t *>(w->host));
    w->host = nullptr; w->dev = nullptr;
}

// ---------------------------------------------------------------------------------------- handle core
OrlgHandle::~OrlgHandle() {
    if (!opened) return;
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (void *b : bufs) (void)hipFree(b);
    if (staging.ptr) (void)hipFree(staging.ptr);
    for (OrlgScratch &s : io)
        if (s.ptr) (void)hipFree(s.ptr);
    for (OrlgScratch &s : extra)
        if (s.ptr) (void)hipFree(s.ptr);
    orlg_err_word_destroy(&err);
    if (own_stream) (void)hipStreamDestroy(stream);
}

int orlg_handle_open(OrlgHandle *h, int device) {
    int ndev = orlg_device_count();
    if (ndev < 1) return fail(ORLG_ERR_NO_DEVICE, "no HIP device visible: liborlg has no CPU path");
    if (device < 0 || device >= ndev) return fail(ORLG_ERR_INVALID, "device %d out of range (have %d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    h->device = device;
    h->opened = true;
    hipDeviceProp_t prop;
    hipError_t er = hipGetDeviceProperties(&prop, device);
    h->num_cu = er == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    er = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (er != hipSuccess) { h->stream = nullptr; return fail(ORLG_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(er)); }
    h->own_stream = true;
    return orlg_err_word_create(&h->err);
}

int orlg_handle_set_stream(OrlgHandle *h, void *hip_stream) {
    if (!h) return fail(ORLG_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->own_stream) { HIP_TRY(hipStreamDestroy(h->stream)); h->own_stream = false; }
    if (hip_stream) {
        h->stream = static_cast<hipStream_t>(hip_stream);
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    return ORLG_OK;
}

int orlg_handle_sync_check(OrlgHandle *h) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->err.host && *h->err.host) return fail(ORLG_ERR_QUEUE_FULL, "%s", h->overflow_message.c_str());
    return ORLG_OK;
}

int orlg_handle_last_kernel(const OrlgHandle *h, char *buf, int32_t cap) {
    if (!h || !buf || cap < 1) return fail(ORLG_ERR_INVALID, "null argument");
    snprintf(buf, (size_t)cap, "%s", h->last_kernel);
    return ORLG_OK;
}

int orlg_kernel_lds(const void *kernel, size_t bytes) {
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return ORLG_OK;
}
int orlg_handle_resident(OrlgHandle *h, const void *kernel, int block, size_t lds, int *resident) {
    if (*resident > 0) return ORLG_OK;
    int nb = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, lds));
    *resident = (nb > 0 ? nb : 1) * h->num_cu;
    return ORLG_OK;
}
void orlg_handle_note_launch(OrlgHandle *h, const char *name, int grid, int block, size_t lds, int chunks, const char *body) {
    char tail[24] = "", btail[16] = "";
    if (chunks > 0) snprintf(tail, sizeof(tail), " chunks=%d", chunks);
    if (body) snprintf(btail, sizeof(btail), " body=%s", body);
    snprintf(h->last_kernel, sizeof(h->last_kernel), "%s grid=%d block=%d lds=%zu%s%s", name, grid, block, lds, btail, tail);
}

int orlg_handle_alloc_bytes(OrlgHandle *h, void **out, size_t bytes, const void *host, bool zero) {
    HIP_TRY(hipMalloc(out, bytes ? bytes : 16));
    h->bufs.push_back(*out);
    if (host) HIP_TRY(hipMemcpy(*out, host, bytes, hipMemcpyHostToDevice));
    else if (zero) HIP_TRY(hipMemset(*out, 0, bytes));
    return ORLG_OK;
}

int orlg_scratch_grow(OrlgScratch *s, size_t bytes) {
    if (bytes <= s->cap) return ORLG_OK;
    if (s->ptr) HIP_TRY(hipFree(s->ptr));
    s->ptr = nullptr; s->cap = 0;
    HIP_TRY(hipMalloc(&s->ptr, bytes));
    s->cap = bytes;
    return ORLG_OK;
}

int orlg_seed_states(OrlgHandle *h, uint32_t *d_mt, int batch, const uint64_t *seeds, uint64_t base_seed, bool trace) {
    (void)h;
    hipError_t er;
    if (trace) {
        er = hipMemset(d_mt, 0, (size_t)batch * ORLG_MT_N * sizeof(uint32_t));   // (part of the saved state; never read)
    } else {
        std::vector<uint32_t> mt((size_t)batch * ORLG_MT_N);
        for (int i = 0; i < batch; i++) orlg_mt_seed(&mt[(size_t)i * ORLG_MT_N], seeds ? seeds[i] : base_seed + (uint64_t)i);
        er = hipMemcpy(d_mt, mt.data(), mt.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    }
    if (er != hipSuccess) return fail(ORLG_ERR_HIP, "upload of MT19937 states: %s", hipGetErrorString(er));
    return ORLG_OK;
}

int orlg_handle_initial_wait(OrlgHandle *h) {
    hipError_t er = hipStreamSynchronize(h->stream);
    if (er != hipSuccess) return fail(ORLG_ERR_HIP, "initial reset: %s", hipGetErrorString(er));
    if (h->trace.length > 0) h->trace.position = 1;   // (the initial reset drew request 0)
    return ORLG_OK;
}

int orlg_handle_place(OrlgHandle *h, const OrlgOut *slots, int n, size_t count, void **outs, int32_t *out_mask) {
    *out_mask = 0;
    for (int i = 0; i < n; i++) {
        outs[i] = nullptr;
        if (!slots[i].user) continue;
        *out_mask |= 1 << i;
        if (orlg_is_device_ptr(slots[i].user)) {
            outs[i] = slots[i].user;
        } else {
            int rc = orlg_scratch_grow(&h->io[i], count * slots[i].elem);
            if (rc) return rc;
            outs[i] = h->io[i].ptr;
        }
    }
    return ORLG_OK;
}
int orlg_handle_collect(OrlgHandle *h, const OrlgOut *slots, int n, size_t count, void *const *outs, bool *any) {
    for (int i = 0; i < n; i++)
        if (outs[i] && outs[i] != slots[i].user) {
            HIP_TRY(hipMemcpyAsync(slots[i].user, outs[i], count * slots[i].elem, hipMemcpyDeviceToHost, h->stream));
            *any = true;
        }
    return ORLG_OK;
}

int orlg_path_records(const orlg_topology *t, int E, const char *link_fmt, std::vector<OrlgPathRec> *recs) {
    recs->resize(t->num_paths);
    for (int g = 0; g < t->num_paths; g++) {
        OrlgPathRec &r = (*recs)[g];
        memset(&r, 0, sizeof(OrlgPathRec));
        const int h = t->path_hops[g];
        if (h < 1 || h > ORLG_MAX_HOPS || t->path_link_off[g + 1] - t->path_link_off[g] != h)
            return fail(ORLG_ERR_INVALID, "path %d: hops %d not in 1..%d or CSR mismatch", g, h, ORLG_MAX_HOPS);
        r.hops = (uint8_t)h; r.se = (uint8_t)t->path_se[g];
        for (int i = 0; i < h; i++) {
            const int l = t->path_links[t->path_link_off[g] + i];
            if (l < 0 || l >= E) return fail(ORLG_ERR_INVALID, link_fmt, g, l);
            r.link[i] = (uint8_t)l;
        }
        for (int i = h; i < ORLG_MAX_HOPS; i++) r.link[i] = r.link[0];   // the padding rule of OrlgPathRec (orlg_device.h)
    }
    return ORLG_OK;
}

// ---------------------------------------------------------------------------------------- per-environment traffic
int orlg_traffic_check(OrlgTrafficState *ts, const orlg_traffic *tr, int batch, double *arrival, double *holding) {
    if (!tr) return ORLG_OK;
    if (!tr->arrival_lambda || !tr->holding_lambda) return fail(ORLG_ERR_INVALID, "traffic: null rate array");
    if (tr->num_groups < 1 || tr->num_groups > 256) return fail(ORLG_ERR_INVALID, "traffic: num_groups %d not in 1..256", tr->num_groups);
    double best = -1.0;
    for (int i = 0; i < batch; i++) {
        const double a = tr->arrival_lambda[i], h = tr->holding_lambda[i];
        if (!std::isfinite(a) || !std::isfinite(h) || !(a > 0) || !(h > 0))
            return fail(ORLG_ERR_INVALID, "traffic: environment %d has arrival_lambda %g, holding_lambda %g: rates must be finite and positive", i, a, h);
        if (tr->group && (tr->group[i] < 0 || tr->group[i] >= tr->num_groups))
            return fail(ORLG_ERR_INVALID, "traffic: group[%d] = %d not in 0..%d", i, tr->group[i], tr->num_groups - 1);
        if (a / h > best) { best = a / h; *arrival = a; *holding = h; }
    }
    ts->arrival.assign(tr->arrival_lambda, tr->arrival_lambda + batch);
    ts->holding.assign(tr->holding_lambda, tr->holding_lambda + batch);
    if (tr->group) ts->group.assign(tr->group, tr->group + batch);
    ts->num_groups = tr->num_groups;
    return ORLG_OK;
}
int orlg_traffic_upload(OrlgHandle *h, int batch) {
    OrlgTrafficState *ts = &h->traffic;
    int rc = ORLG_OK;
    if (!ts->arrival.empty()) {
        std::vector<OrlgRates> r((size_t)batch);
        for (int i = 0; i < batch; i++) { r[i].arrival_lambda = ts->arrival[i]; r[i].holding_lambda = ts->holding[i]; }
        rc = orlg_handle_upload(h, &ts->d_rates, r.data(), r.size());
    }
    if (!rc && !ts->group.empty()) rc = orlg_handle_upload(h, &ts->d_group, ts->group.data(), (size_t)batch);
    return rc;
}
int orlg_traffic_get(const OrlgTrafficState *ts, int batch, double arrival_lambda, double holding_lambda, double *arrival,
                     double *holding, int32_t *group) {
    for (int i = 0; i < batch; i++) {
        if (arrival) arrival[i] = ts->arrival.empty() ? arrival_lambda : ts->arrival[i];
        if (holding) holding[i] = ts->holding.empty() ? holding_lambda : ts->holding[i];
        if (group) group[i] = ts->group.empty() ? 0 : ts->group[i];
    }
    return ORLG_OK;
}

// ---------------------------------------------------------------------------------------- request traces
int orlg_trace_check(OrlgTraceState *st, OrlgTrafficState *ts, const orlg_trace *tr, int batch, int N, int NBR,
                     const int32_t *bit_rates, bool cont, double *arrival, double *holding) {
    if (!tr) return fail(ORLG_ERR_INVALID, "trace: null argument");
    if (!tr->arrival || !tr->holding || !tr->src || !tr->dst || !tr->bit_rate) return fail(ORLG_ERR_INVALID, "trace: null array");
    if (tr->length < 2) return fail(ORLG_ERR_INVALID, "trace: length %lld, a trace has at least 2 requests per environment", (long long)tr->length);
    if (tr->length > 0x7fffffffll || (double)tr->length * batch > 4.0e9)
        return fail(ORLG_ERR_INVALID, "trace: %lld requests x %d environments is more than the device index holds", (long long)tr->length, batch);
    if (tr->group) {
        if (tr->num_groups < 1 || tr->num_groups > 256) return fail(ORLG_ERR_INVALID, "trace: num_groups %d not in 1..256", tr->num_groups);
        for (int i = 0; i < batch; i++)
            if (tr->group[i] < 0 || tr->group[i] >= tr->num_groups)
                return fail(ORLG_ERR_INVALID, "trace: group[%d] = %d not in 0..%d", i, tr->group[i], tr->num_groups - 1);
        ts->group.assign(tr->group, tr->group + batch);
        ts->num_groups = tr->num_groups;
    }
    const size_t n = (size_t)tr->length;
    st->req.assign((size_t)batch * n, 0u);
    // the release times of the requests in progress, earliest first (a binary heap), and how many of them every ordered pair has
    std::vector<double> heap_t;
    std::vector<int32_t> heap_pair, pair_cnt((size_t)N * N, 0);
    int peak = 0, pair_peak = 0;
    double hold_sum = 0.0;
    auto heap_less = [&](size_t a, size_t b) { return heap_t[a] < heap_t[b]; };
    for (int i = 0; i < batch; i++) {
        heap_t.clear(); heap_pair.clear();
        std::fill(pair_cnt.begin(), pair_cnt.end(), 0);
        double prev = 0.0;
        for (size_t j = 0; j < n; j++) {
            const size_t at = (size_t)i * n + j;
            const double a = tr->arrival[at], h = tr->holding[at];
            const int s = tr->src[at], d = tr->dst[at], br = tr->bit_rate[at];
            if (!std::isfinite(a) || a < 0) return fail(ORLG_ERR_INVALID, "trace: environment %d, request %zu: arrival %g is not a finite time >= 0", i, j, a);
            if (a < prev) return fail(ORLG_ERR_INVALID, "trace: environment %d, request %zu: arrival %.17g before its predecessor's %.17g", i, j, a, prev);
            if (!std::isfinite(h) || h < 0) return fail(ORLG_ERR_INVALID, "trace: environment %d, request %zu: holding %g is not a finite time >= 0", i, j, h);
            if (s < 0 || s >= N || d < 0 || d >= N) return fail(ORLG_ERR_INVALID, "trace: environment %d, request %zu: node pair (%d, %d) outside 0..%d", i, j, s, d, N - 1);
            if (s == d) return fail(ORLG_ERR_INVALID, "trace: environment %d, request %zu: source and destination are both %d", i, j, s);
            int bri = -1;
            if (cont) {
                if (br >= bit_rates[0] && br <= bit_rates[NBR - 1]) bri = br - bit_rates[0];
            } else {
                for (int b = 0; b < NBR && bri < 0; b++)
                    if (bit_rates[b] == br) bri = b;
            }
            if (bri < 0 && cont)
                return fail(ORLG_ERR_INVALID, "trace: environment %d, request %zu: bit rate %d outside the bounds %d..%d", i, j, br, bit_rates[0], bit_rates[NBR - 1]);
            if (bri < 0) return fail(ORLG_ERR_INVALID, "trace: environment %d, request %zu: bit rate %d is not one of the config's bit rates", i, j, br);
            st->req[at] = (uint32_t)s | ((uint32_t)d << 8) | ((uint32_t)bri << 16);
            prev = a;
            hold_sum += h;
            // requests whose interval ended before this arrival leave; the interval is closed, an end AT the arrival stays
            while (!heap_t.empty() && heap_t[0] < a) {
                pair_cnt[heap_pair[0]] -= 1;
                // pop the root
                const size_t last = heap_t.size() - 1;
                heap_t[0] = heap_t[last]; heap_pair[0] = heap_pair[last];
                heap_t.pop_back(); heap_pair.pop_back();
                size_t k = 0;
                for (;;) {
                    size_t l = 2 * k + 1, r = l + 1, m = k;
                    if (l < heap_t.size() && heap_less(l, m)) m = l;
                    if (r < heap_t.size() && heap_less(r, m)) m = r;
                    if (m == k) break;
                    std::swap(heap_t[k], heap_t[m]); std::swap(heap_pair[k], heap_pair[m]);
                    k = m;
                }
            }
            heap_t.push_back(a + h); heap_pair.push_back(s * N + d);
            for (size_t k = heap_t.size() - 1; k > 0;) {
                const size_t par = (k - 1) / 2;
                if (!heap_less(k, par)) break;
                std::swap(heap_t[k], heap_t[par]); std::swap(heap_pair[k], heap_pair[par]);
                k = par;
            }
            const int pc = ++pair_cnt[s * N + d];
            if ((int)heap_t.size() > peak) peak = (int)heap_t.size();
            if (pc > pair_peak) pair_peak = pc;
        }
    }
    st->length = tr->length;
    st->position = 0;
    st->peak = peak; st->pair_peak = pair_peak;
    st->mean_holding = hold_sum / ((double)batch * (double)n);
    *arrival = 1.0; *holding = st->mean_holding > 0 ? 1.0 / st->mean_holding : 1.0;
    return ORLG_OK;
}
int orlg_trace_upload(OrlgHandle *h, const orlg_trace *tr, int batch) {
    OrlgTraceState *st = &h->trace;
    const size_t cnt = (size_t)batch * (size_t)st->length;
    int rc = orlg_handle_upload(h, &st->d_arrival, tr->arrival, cnt);
    if (!rc) rc = orlg_handle_upload(h, &st->d_holding, tr->holding, cnt);
    if (!rc) rc = orlg_handle_upload(h, &st->d_req, st->req.data(), cnt);
    if (!rc) rc = orlg_handle_alloc(h, &st->d_tail, 2);
    std::vector<uint32_t>().swap(st->req);
    return rc;
}
int orlg_trace_admit(const OrlgTraceState *st, int n_steps) {
    if (st->length > 0 && st->position + (int64_t)n_steps > st->length)
        return fail(ORLG_ERR_INVALID, "trace: %d steps from position %lld would draw past the trace's %lld requests per environment "
                                      "(a trace of n requests allows n - 1 steps after a full reset)", n_steps, (long long)st->position, (long long)st->length);
    return ORLG_OK;
}
int orlg_trace_tail_store(OrlgTraceState *st, hipStream_t stream) {
    if (st->length <= 0) return ORLG_OK;
    const int64_t tail[2] = {st->position, st->length};
    HIP_TRY(hipMemcpyAsync(st->d_tail, tail, 16, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return ORLG_OK;
}
int orlg_trace_tail_check(const OrlgTraceState *st, const void *tail_ptr) {
    if (st->length <= 0) return ORLG_OK;
    int64_t tail[2] = {0, 0};
    HIP_TRY(hipMemcpy(tail, tail_ptr, 16, hipMemcpyDefault));
    if (tail[1] != st->length || tail[0] < 1 || tail[0] > st->length)
        return fail(ORLG_ERR_INVALID, "snapshot of a trace of %lld requests at position %lld: this handle's trace has %lld (nothing was loaded)",
                    (long long)tail[1], (long long)tail[0], (long long)st->length);
    return ORLG_OK;
}
int orlg_trace_tail_load(OrlgTraceState *st, hipStream_t stream) {
    if (st->length <= 0) return ORLG_OK;
    int64_t tail[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(tail, st->d_tail, 16, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (tail[1] != st->length || tail[0] < 1 || tail[0] > st->length)
        return fail(ORLG_ERR_INVALID, "snapshot of a trace of %lld requests at position %lld: this handle's trace has %lld",
                    (long long)tail[1], (long long)tail[0], (long long)st->length);
    st->position = tail[0];
    return ORLG_OK;
}

// ---------------------------------------------------------------------------------------- MT19937 seeding
// CPython _randommodule.c: random.Random(n) -> init_by_array(32-bit little-endian chunks of abs(n)).
void orlg_mt_seed(uint32_t *mt, uint64_t seed) {
    uint32_t key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
    int len = key[1] ? 2 : 1;
    mt[0] = 19650218u;
    for (int i = 1; i < ORLG_MT_N; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    int i = 1, j = 0;
    for (int k = ORLG_MT_N > len ? ORLG_MT_N : len; k; k--) {
        mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
        i++; j++;
        if (i >= ORLG_MT_N) { mt[0] = mt[ORLG_MT_N - 1]; i = 1; }
        if (j >= len) j = 0;
    }
    for (int k = ORLG_MT_N - 1; k; k--) {
        mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
        i++;
        if (i >= ORLG_MT_N) { mt[0] = mt[ORLG_MT_N - 1]; i = 1; }
    }
    mt[0] = 0x80000000u;
}

// ---------------------------------------------------------------------------------------- pointers
int orlg_is_device_ptr(const void *ptr) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// A pointer the kernels can use as it is: device / managed memory, or PINNED host memory (hipHostMalloc, torch's pin_memory),
// which the device reaches over the bus -- returns the device-side alias, nullptr for pageable host memory
void *orlg_device_alias(const void *ptr) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) return const_cast<void *>(ptr);
    if (a.type == hipMemoryTypeHost && a.devicePointer) return a.devicePointer;
    return nullptr;
}

// ---------------------------------------------------------------------------------------- checkpoint / resume
// The whole simulation state of a handle is a handful of flat device arrays: a snapshot is their concatenation.
int orlg_state_copy(const std::vector<OrlgStatePart> &parts, void *buffer, bool save, int device, hipStream_t stream) {
    HIP_TRY(hipSetDevice(device));
    unsigned char *b = static_cast<unsigned char *>(buffer);
    for (const OrlgStatePart &sp : parts) {
        if (save) HIP_TRY(hipMemcpyAsync(b, sp.ptr, sp.bytes, hipMemcpyDefault, stream));
        else HIP_TRY(hipMemcpyAsync(sp.ptr, b, sp.bytes, hipMemcpyDefault, stream));
        b += sp.bytes;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return ORLG_OK;
}
int64_t orlg_handle_state_size(const std::vector<OrlgStatePart> &parts) {
    int64_t n = 0;
    for (const OrlgStatePart &sp : parts) n += (int64_t)sp.bytes;
    return n;
}
int orlg_handle_state_save(OrlgHandle *h, const std::vector<OrlgStatePart> &parts, void *buffer) {
    if (!h || !buffer) return fail(ORLG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    int rc = orlg_trace_tail_store(&h->trace, h->stream);
    if (rc) return rc;
    return orlg_state_copy(parts, buffer, true, h->device, h->stream);
}
int orlg_handle_state_load(OrlgHandle *h, const std::vector<OrlgStatePart> &parts, const void *buffer) {
    if (!h || !buffer) return fail(ORLG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    if (h->trace.length > 0) {   // the position's 16 bytes, checked in the caller's buffer before anything is copied
        size_t off = 0;
        for (const OrlgStatePart &sp : parts) {
            if (sp.ptr == h->trace.d_tail) break;
            off += sp.bytes;
        }
        int rc = orlg_trace_tail_check(&h->trace, static_cast<const unsigned char *>(buffer) + off);
        if (rc) return rc;
    }
    int rc = orlg_state_copy(parts, const_cast<void *>(buffer), false, h->device, h->stream);
    if (rc) return rc;
    rc = orlg_trace_tail_load(&h->trace, h->stream);
    if (rc) return rc;
    *h->err.host = 0;
    return ORLG_OK;
}

// ---------------------------------------------------------------------------------------- C ABI: the library itself
extern "C" {
int orlg_abi_version(void) { return ORLG_ABI_VERSION; }
const char *orlg_last_error(void) { return g_err.c_str(); }
int orlg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}
}  // extern "C"
