// orlg_api_step.hip -- the step of the RMSA C API (include/orlg.h): the launch of the step kernels (launch_rmsa, which create and reset
// use as well: the wave kernels' one launch_wave and the group kernel's launch_rmsa_group), one launch of a resolved call (rmsa_step; what a call resolves to and what
// refuses it: orlg_step_call.h), the orlg_step* entries, and the GN-model gate a step checks against with its setters.
#include "orlg_rmsa_host.h"
#include "orlg_step_call.h"
#include "orlg_qdesc.h"

// ---------------------------------------------------------------------------------------- launches
// the kernels live in per-W objects (orlg_inst_wave.hip / orlg_inst_group.hip), found by key: orlg_pick (orlg_variants.h)
typedef orlg_rmsa_kernel_t rmsa_kernel_t;

// the tooling environment of a launch
static OrlgGroupOverrides group_overrides() {
    const char *wpb = getenv("ORLG_GROUP_WPB"), *chunks = getenv("ORLG_GROUP_CHUNKS");
    return {getenv("ORLG_NO_DEFER") != nullptr, getenv("ORLG_NO_CHUNKS") != nullptr, getenv("ORLG_NO_LEAN") != nullptr,
            wpb ? atoi(wpb) : 0, chunks ? atoi(chunks) : 0};
}

// ---- the step kernel with four environments per wave: first-fit policies and external (path, slot) actions.  What is launched is
// decided in orlg_group_plan.h; here it is done
// a launch of orlg_step_window under the rule MOST_USED or the route BEST_WINDOW: the USAGE instantiations (orlg_usage.h)
static bool usage_launch(const OrlgParams &p) {
    return (p.out_mask & ORLG_OUT_ASSIGN_BIT) != 0 && (p.assign == ORLG_ASSIGN_MOST_USED || p.policy == ORLG_POLICY_BEST_WINDOW);
}

static int launch_rmsa_group(orlg_env *e, const OrlgParams &p, const OrlgGroupOverrides &ov) {
    OrlgGroupChoice c = orlg_group_choose(e->group, {p.B, p.n_steps, p.stats_level, p.policy, p.out_mask, p.br_width, p.NBR, e->min_slots}, ov, e->num_cu);
    const OrlgGroupLayout &l = e->group[c.kind];
    const bool df = c.kind == ORLG_GROUP_DEFER;
    const bool trace = p.tr_arrival != nullptr;   // a request trace: the instantiations that replay it
    const bool traffic = !trace && p.rates != nullptr;   // per-environment rates: the instantiations that read them
    const bool cause = (p.out_mask & ORLG_OUT_CAUSE_BIT) != 0;   // the blocking cause: the plain kind with the classifier (the plan chose it)
    const bool assign = (p.out_mask & ORLG_OUT_ASSIGN_BIT) != 0;   // an assignment rule: the plain kind with the rules (the plan chose it)
    const bool cut = assign && p.assign == ORLG_ASSIGN_MIN_CUT;   // ... the fewest-cuts window: the CUT instantiations
    const bool usage = usage_launch(p);   // ... MOST_USED / BEST_WINDOW: the USAGE instantiations, with their prefix sums behind the wave regions
    const OrlgGroupKey key = {p.stats_level, c.kind == ORLG_GROUP_HBMQ, df, traffic, trace, cause, assign, cut, usage};
    rmsa_kernel_t k = orlg_pick(e->W, key);
    if (!k) return fail(ORLG_ERR_INVALID, "no kernel for W=%d", e->W);
    if (usage) {
        c.wpb = orlg_group_usage_wpb(l, c.wpb, e->W);
        if (c.wpb < 1)
            return fail(ORLG_ERR_INVALID, "step_kernel \"group\": one wave's four environments (%d B) and their slot-usage prefix sums (%d B) do not "
                                          "fit the LDS next to the tables (%d B); use step_kernel \"wave\" or \"auto\" for this policy",
                        l.wave_bytes, 4 * ORLG_USAGE_BYTES(e->W), l.shared_bytes);
        c.lds_bytes = orlg_group_lds(l.shared_bytes, c.wpb, l.wave_bytes + 4 * ORLG_USAGE_BYTES(e->W));
    }
    if (df && !e->llog)
        if (int rc = orlg_handle_alloc(e, &e->llog, (size_t)p.B * p.E * ORLG_LLOG_CAP)) return rc;
    if (int rc = orlg_kernel_lds(reinterpret_cast<const void *>(k), usage ? c.lds_bytes : orlg_group_lds(l.shared_bytes, l.wpb_max, l.wave_bytes))) return rc;
    int *resident = usage ? &e->group_usage_resident[c.wpb] : &e->group_resident[c.kind][c.wpb];
    if (int rc = orlg_handle_resident(e, reinterpret_cast<const void *>(k), ORLG_WAVE * c.wpb, c.lds_bytes, resident)) return rc;
    const OrlgGroupTickets t = orlg_group_tickets(c, p.B, p.n_steps, *resident, ov);
    if (t.n_chunks > 1) {
        if (!e->progress)
            if (int rc = orlg_handle_alloc(e, &e->progress, (size_t)p.B / 4 + 1)) return rc;
        HIP_TRY(hipMemsetAsync(e->progress, 0, (size_t)t.n_quads * sizeof(uint32_t), e->stream));
    }
    OrlgParams q = p;
    q.llog = df ? e->llog : nullptr;
    q.g_lstat = l.lstat; q.g_lint = l.lint; q.g_qtime = l.qtime; q.g_qdesc = l.qdesc; q.g_wave_bytes = l.wave_bytes;
    q.g_lean = c.lean;
    q.ticket_base = e->ticket_base; q.ticket_stride = c.ticket_stride;
    q.n_chunks = t.n_chunks; q.chunk_steps = t.chunk_steps; q.progress = t.n_chunks > 1 ? e->progress : nullptr;
    e->ticket_base += t.ticket_advance;
    hipLaunchKernelGGL(k, dim3(t.nblocks), dim3(ORLG_WAVE * c.wpb), c.lds_bytes, e->stream, q);
    HIP_TRY(hipGetLastError());
    orlg_handle_launched(e, key, t.nblocks, ORLG_WAVE * c.wpb, c.lds_bytes, t.n_chunks, c.lean ? "lean" : "full");
    return ORLG_OK;
}

static bool group_kernel_serves(const orlg_env *e, const OrlgParams &p) {
    if (e->group_mode == ORLG_KERNEL_WAVE || p.mode != ORLG_MODE_STEP || p.gn) return false;   // (a gated handle: the wave kernel's GN instantiations)
    if (e->group_mode == ORLG_KERNEL_GROUP) return true;
    // (a USAGE launch whose prefix sums the LDS does not hold next to one wave's environments: the wave kernel)
    if (usage_launch(p) && orlg_group_usage_wpb(e->group[ORLG_GROUP_PLAIN], 1, e->W) < 1) return false;
    // AUTO: this kernel once the batch exceeds what the wave-per-environment kernel keeps resident (4096 environments on
    // MI355X) -- long launches (B = 65 536: 1140 vs 630 M env-steps/s) and launches of one step alike (B = 32 768, DeepRMSA
    // shape: 0.145 vs 0.161 ms per step + observation); at or below it the wave-per-environment kernel has the shorter step
    // (B = 4096: 630 vs 440 M).
    return p.B > e->resident_blocks * e->waves_per_block;
}

// ---- the wave-per-environment step kernels: what is launched is decided in orlg_wave_plan.h; here it is done
// the plain wave-per-environment step kernel
static rmsa_kernel_t step_kernel(int W, int stats) { return orlg_pick(W, OrlgWaveKey{ORLG_WAVE_KERNEL(orlg_rmsa_kernel), stats, false}); }

// What a step entry resolved beyond the call (rmsa_step): the family its launch runs -- orlg_step_max_margin's calls are MM, every other
// entry leaves the plan to find it (a handle whose gate chooses the modulation: AM) -- with the workgroup of an MM launch (mm_geometry)
// and where the kernel's second argument points: gn_window_margin_db (OrlgMmArgs), gn_se (OrlgAmArgs); nullptr = not asked for
struct WaveFamily {
    OrlgWaveFamily family = ORLG_WAVE_PLAIN;
    OrlgWaveShape mm = {};
    double *window_margin = nullptr;
    uint8_t *se = nullptr;
};
// one launch: the kernel and the name it reports, the kernel's second argument (nullptr: it has none), the workgroup, where the
// resident workgroups of this kernel and shape are kept, and the log of a DEFER instantiation (nullptr for any other)
struct WaveLaunch {
    const void *kernel = nullptr;
    char name[96] = "";
    const void *arg2 = nullptr;
    int wpu = 0;
    size_t lds = 0;
    int *resident = nullptr;
    uint4 *llog = nullptr;
};
template <typename Key>
static int wave_kernel(const orlg_env *e, const Key &key, WaveLaunch *w) {
    w->kernel = reinterpret_cast<const void *>(orlg_pick(e->W, key));
    if (!w->kernel) return fail(ORLG_ERR_INVALID, "no kernel for W=%d", e->W);
    orlg_kernel_name(w->name, sizeof(w->name), e->W, key);
    return ORLG_OK;
}
static int launch_wave(orlg_env *e, const OrlgParams &p, const WaveLaunch &w) {
    if (int rc = orlg_kernel_lds(w.kernel, w.lds)) return rc;
    if (int rc = orlg_handle_resident(e, w.kernel, ORLG_WAVE * w.wpu, w.lds, w.resident)) return rc;
    const OrlgWaveGrid g = orlg_wave_grid(p.B, w.wpu, *w.resident, p.mode, p.n_steps);
    OrlgParams q = p;
    q.llog = w.llog;
    q.ticket_base = e->ticket_base;
    q.ticket_stride = g.ticket_stride;
    e->ticket_base += g.ticket_advance;
    void *args[] = {&q, const_cast<void *>(w.arg2)};
    (void)hipLaunchKernel(w.kernel, dim3(g.nblocks), dim3(ORLG_WAVE * w.wpu), args, w.lds, e->stream);
    HIP_TRY(hipGetLastError());
    orlg_handle_note_launch(e, w.name, g.nblocks, ORLG_WAVE * w.wpu, w.lds, 0, nullptr);
    return ORLG_OK;
}

static int launch_rmsa_family(orlg_env *e, const OrlgParams &p, const WaveFamily &f) {
    const OrlgGroupOverrides ov = group_overrides();
    const OrlgWaveChoice c = orlg_wave_choose({p.mode, p.policy, p.K, p.stats_level, p.n_steps, (int)p.out_mask, p.assign, p.gn != nullptr,
                                               p.gn_adaptive != 0, e->gn_protect, f.family == ORLG_WAVE_MM, ov.no_defer});
    WaveLaunch w;
    w.wpu = e->waves_per_block;
    w.lds = e->lds_block_bytes;
    // orlg_rmsa_mm_kernel and orlg_rmsa_am_kernel: a second kernel argument, and the resident workgroups of their own kernel and shape
    if (c.family == ORLG_WAVE_MM) {
        if (int rc = wave_kernel(e, c.mm, &w)) return rc;
        const OrlgMmArgs a = {f.window_margin, e->gn_protect ? 1 : 0, 0};
        w.arg2 = &a; w.wpu = f.mm.wpu; w.lds = f.mm.lds;
        w.resident = &e->mm_resident[p.stats_level][c.mm.CAUSE ? 1 : 0];
        return launch_wave(e, p, w);
    }
    if (c.family == ORLG_WAVE_AM) {   // (the handle's own workgroup: it needs no LDS beyond the wave regions)
        if (int rc = wave_kernel(e, c.am, &w)) return rc;
        const OrlgAmArgs a = {f.se};
        w.arg2 = &a;
        w.resident = &e->am_resident[p.stats_level];
        return launch_wave(e, p, w);
    }
    if (int rc = wave_kernel(e, c.key, &w)) return rc;
    // Every launch of this family sizes its grid from resident_blocks, asked once for the plain step kernel at the handle's workgroup --
    // a GN, CAUSE or ASSIGN launch too, and a USAGE launch of fewer waves per workgroup (any grid is correct; other code reads the value)
    if (e->resident_blocks <= 0) {
        const void *ks = reinterpret_cast<const void *>(step_kernel(e->W, p.stats_level));
        int rc = orlg_kernel_lds(ks, e->lds_block_bytes);
        if (!rc) rc = orlg_handle_resident(e, ks, ORLG_WAVE * w.wpu, e->lds_block_bytes, &e->resident_blocks);
        if (rc) return rc;
    }
    w.resident = &e->resident_blocks;
    if (group_kernel_serves(e, p)) return launch_rmsa_group(e, p, ov);   // (after the key is picked: a W without kernels is refused first)
    // (a USAGE launch: the waves' prefix sums of the slot usage lie behind the wave regions, asked for here and by no other launch;
    // where the handle's workgroup fills the LDS, such a launch runs with as many waves per workgroup as still fit)
    if (c.key.USAGE) {
        const OrlgWaveShape u = orlg_wave_extra_lds(p.l_shared_bytes, p.l_wave_bytes, ORLG_USAGE_BYTES(e->W), w.wpu);
        if (!u.wpu)
            return fail(ORLG_ERR_INVALID, "tables, one environment and its slot-usage prefix sums (%zu B) exceed the 160 KiB LDS", u.lds);
        w.wpu = u.wpu; w.lds = u.lds;
    }
    if (c.key.DEFER) {
        if (!e->llog)
            if (int rc = orlg_handle_alloc(e, &e->llog, (size_t)p.B * p.E * ORLG_LLOG_CAP)) return rc;
        w.llog = e->llog;
    }
    return launch_wave(e, p, w);
}
int launch_rmsa(orlg_env *e, const OrlgParams &p) { return launch_rmsa_family(e, p, {}); }

// the workgroup of orlg_rmsa_mm_kernel (orlg_inst_gnmm.hip): the handle's wave regions and, behind them, up16(4 Q) bytes
// per wave for the compacted services of the path under evaluation.  Refused where one wave does not fit
static int mm_geometry(const orlg_env *e, OrlgWaveShape *m) {
    *m = orlg_wave_extra_lds(e->p.l_shared_bytes, e->p.l_wave_bytes, ((size_t)e->p.Q * 4 + 15) & ~(size_t)15, e->waves_per_block);
    if (!m->wpu)
        return fail(ORLG_ERR_INVALID, "orlg_step_max_margin: tables, one environment and the ring of its %d compacted services (%zu B) exceed the 160 KiB LDS",
                    e->p.Q, m->lds);
    return ORLG_OK;
}

extern "C" {
/* launch geometry of the step kernel: out[0] waves (envs) per workgroup, out[1] LDS bytes per workgroup,
 * out[2] workgroups resident per CU according to hipOccupancyMaxActiveBlocksPerMultiprocessor, out[3] W */
int orlg_launch_info(orlg_env *e, int32_t *out) {
    if (!e || !out) return fail(ORLG_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(e->device));
    rmsa_kernel_t k = step_kernel(e->W, e->p.stats_level);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)e->lds_block_bytes));
    int nb = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void *>(k), ORLG_WAVE * e->waves_per_block,
                                                         e->lds_block_bytes));
    out[0] = e->waves_per_block; out[1] = (int32_t)e->lds_block_bytes; out[2] = nb; out[3] = e->W;
    return ORLG_OK;
}
}  // extern "C"

// ---------------------------------------------------------------------------------------- the step
// the outputs of a step beyond orlg_step_io (nullptr = not asked for): gn_gsnr_db, block_cause and cause_counts of orlg_step_diag,
// gn_neighbour_margin_db of orlg_step_gn_protect, gn_window_margin_db of orlg_step_max_margin
struct StepExtras {
    double *gsnr = nullptr;
    uint8_t *cause = nullptr;
    int32_t *counts = nullptr;
    double *margin = nullptr;
    double *wmargin = nullptr;
    uint8_t *se = nullptr;   // gn_se of orlg_step_modulation
};
static StepExtras step_extras(const struct orlg_step_diag *diag, double *margin = nullptr) {
    StepExtras x;
    if (diag) { x.gsnr = diag->gn_gsnr_db; x.cause = diag->block_cause; x.counts = diag->cause_counts; }
    x.margin = margin;
    return x;
}
// Where the kernel writes one of them: memory the device reaches is written in place, any other through the handle's buffer `slot`
// and copied to the caller after the launch.  What counts as reachable is the slot's: with `alias`, device memory and pinned host
// memory, written through its device alias (orlg_device_alias); without, device memory alone (orlg_is_device_ptr)
struct ExtraOut {
    void *user;
    size_t bytes;
    int slot;
    bool alias;
    void *dev = nullptr;
    bool staged = false;
};
static int place_extra(orlg_env *e, ExtraOut *o) {
    if (!o->user) return ORLG_OK;
    o->dev = o->alias ? orlg_device_alias(o->user) : orlg_is_device_ptr(o->user) ? o->user : nullptr;
    if (o->dev) return ORLG_OK;
    if (int rc = orlg_scratch_grow(&e->extra[o->slot], o->bytes)) return rc;
    o->dev = e->extra[o->slot].ptr;
    o->staged = true;
    return ORLG_OK;
}

// one launch of n_steps steps of a call that orlg_step_call has resolved: the live part of every step entry.  fam.family MM: the call
// is orlg_step_max_margin's (orlg_step_mm_call resolved it, mm_geometry found its workgroup) and launches orlg_rmsa_mm_kernel; AM: the
// call is orlg_step_modulation's (call.policy is the device's ORLG_POLICY_*_AM) and launches orlg_rmsa_am_kernel with gn_se
static int rmsa_step(orlg_env *e, const OrlgStepCall &call, int32_t n_steps, const int32_t *actions, int32_t auto_reset,
                     const orlg_step_io *io, const StepExtras &x, WaveFamily fam = {}) {
    const int32_t policy = call.policy;
    const bool am = fam.family == ORLG_WAVE_AM;
    const bool ext = am ? policy == ORLG_POLICY_PATH_AM_EXT || policy == ORLG_POLICY_EXT_AM
                        : policy == ORLG_POLICY_EXTERNAL || policy == ORLG_POLICY_DEEPRMSA_EXTERNAL || policy == ORLG_POLICY_PATH_FF_EXTERNAL;
    if (ext && (!actions || n_steps != 1)) return fail(ORLG_ERR_INVALID, "external actions need an action array and n_steps == 1");
    if (int rc = orlg_trace_admit(&e->trace, n_steps)) return rc;   // before anything is launched or copied
    HIP_TRY(hipSetDevice(e->device));
    OrlgParams p = e->p;
    p.mode = ORLG_MODE_STEP; p.n_steps = n_steps; p.policy = policy; p.auto_reset = auto_reset;
    if (ext) {
        size_t n = (size_t)p.B * (am ? (policy == ORLG_POLICY_EXT_AM ? 3 : 1) : policy == ORLG_POLICY_EXTERNAL ? 2 : 1);
        if (const void *da = orlg_device_alias(actions)) {   // device memory, or pinned host memory read over the bus
            p.actions = static_cast<const int32_t *>(da);
        } else {
            int rc = orlg_scratch_grow(&e->extra[X_ACTIONS], n * sizeof(int32_t));
            if (rc) return rc;
            p.actions = static_cast<const int32_t *>(e->extra[X_ACTIONS].ptr);
            HIP_TRY(hipMemcpyAsync(e->extra[X_ACTIONS].ptr, actions, n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
        }
    }
    // outputs: write straight into device pointers, stage host pointers
    const size_t cnt = (size_t)n_steps * p.B;
    const OrlgOut slots[ORLG_NUM_OUTS] = {
        {io ? io->act_path : nullptr, 4},   {io ? io->act_slot : nullptr, 4},  {io ? io->accepted : nullptr, 1},
        {io ? io->done : nullptr, 1},       {io ? io->reward : nullptr, 8},    {io ? io->request : nullptr, 16},
        {io ? io->arrival : nullptr, 8},    {io ? io->holding : nullptr, 8},   {io ? io->network_compactness : nullptr, 8},
        {io ? io->network_compactness_difference : nullptr, 8},
        {io ? io->avg_link_compactness : nullptr, 8},   {io ? io->avg_link_utilization : nullptr, 8}};
    int rc = orlg_handle_place(e, slots, ORLG_NUM_OUTS, cnt, p.outs, &p.out_mask);
    if (rc) return rc;
    ExtraOut extra[6] = {{x.gsnr, cnt * sizeof(double), X_GSNR, true}, {x.cause, cnt, X_CAUSE, false},
                         {x.counts, (size_t)p.B * ORLG_NUM_CAUSES * sizeof(int32_t), X_CAUSE_COUNTS, false},
                         {x.margin, cnt * sizeof(double), X_MARGIN, false}, {x.wmargin, cnt * sizeof(double), X_WINDOW_MARGIN, false},
                         {x.se, cnt, X_SE, false}};
    for (ExtraOut &o : extra)
        if ((rc = place_extra(e, &o))) return rc;
    p.o_gsnr = static_cast<double *>(extra[0].dev);
    p.o_cause = static_cast<uint8_t *>(extra[1].dev);
    p.o_cause_counts = static_cast<int32_t *>(extra[2].dev);
    p.o_margin = static_cast<double *>(extra[3].dev);
    if (x.gsnr && !p.gn) HIP_TRY(hipMemsetAsync(p.o_gsnr, 0xff, extra[0].bytes, e->stream));   // no gate, no check: all NaN
    // block_cause / cause_counts: the launch runs a CAUSE instantiation (ORLG_OUT_CAUSE_BIT); the counts are zeroed on the stream
    if (x.cause || x.counts) p.out_mask |= ORLG_OUT_CAUSE_BIT;
    if (x.counts) HIP_TRY(hipMemsetAsync(p.o_cause_counts, 0, extra[2].bytes, e->stream));
    // gn_neighbour_margin_db: written by a protecting handle's kernels; every other handle ran no second check -- all NaN
    if (x.margin && !(p.gn && e->gn_protect)) HIP_TRY(hipMemsetAsync(p.o_margin, 0xff, extra[3].bytes, e->stream));
    p.assign = call.assign;
    if (call.assign != ORLG_ASSIGN_FIRST) p.out_mask |= ORLG_OUT_ASSIGN_BIT;   // the launch runs an ASSIGN instantiation
    fam.window_margin = static_cast<double *>(extra[4].dev);
    fam.se = static_cast<uint8_t *>(extra[5].dev);
    rc = launch_rmsa_family(e, p, fam);
    if (rc) return rc;
    if (e->trace.length > 0) e->trace.position += n_steps;
    bool any = false;
    rc = orlg_handle_collect(e, slots, ORLG_NUM_OUTS, cnt, p.outs, &any);
    if (rc) return rc;
    for (const ExtraOut &o : extra)
        if (o.staged) {
            HIP_TRY(hipMemcpyAsync(o.user, o.dev, o.bytes, hipMemcpyDeviceToHost, e->stream));
            any = true;
        }
    if (any) SYNC_CHECK(e);
    return ORLG_OK;
}
// every step entry: the call resolved against the handle's gate (orlg_step_call.h: the checks, in the order they refuse), then launched
static int step_entry(orlg_env *e, OrlgStepEntry entry, int32_t policy, int32_t rule, int32_t gn_mode, int32_t n_steps, const int32_t *actions,
                      int32_t auto_reset, const orlg_step_io *io, const StepExtras &x) {
    if (!e) return fail(ORLG_ERR_INVALID, "null handle");
    OrlgStepCall call;
    if (int rc = orlg_step_call({entry, policy, rule, gn_mode, n_steps, e->p.gn != nullptr, e->gn_protect}, &call)) return rc;
    // a handle whose gate chooses the modulation: what its one kernel does not hold is refused
    if (e->p.gn_adaptive) {
        if (entry == ORLG_ENTRY_RULE_GN)
            return fail(ORLG_ERR_INVALID, "orlg_step_rule_gn: the handle's gate chooses the modulation (orlg_set_gn_modulation), and no assignment rule runs behind it yet");
        if (x.cause || x.counts)
            return fail(ORLG_ERR_INVALID, "block_cause / cause_counts: the handle's gate chooses the modulation (orlg_set_gn_modulation), and its step kernel holds no classifier yet");
    }
    return rmsa_step(e, call, n_steps, actions, auto_reset, io, x);
}
extern "C" {
int orlg_step(orlg_env *e, int32_t policy, int32_t n_steps, const int32_t *actions, int32_t auto_reset, const orlg_step_io *io) {
    return step_entry(e, ORLG_ENTRY_PLAIN, policy, 0, 0, n_steps, actions, auto_reset, io, {});
}
int orlg_step_gn(orlg_env *e, int32_t policy, int32_t n_steps, const int32_t *actions, int32_t auto_reset, const orlg_step_io *io,
                 double *gn_gsnr_db) {
    StepExtras x;
    x.gsnr = gn_gsnr_db;
    return step_entry(e, ORLG_ENTRY_PLAIN, policy, 0, 0, n_steps, actions, auto_reset, io, x);
}
int orlg_step_diag(orlg_env *e, int32_t policy, int32_t n_steps, const int32_t *actions, int32_t auto_reset, const orlg_step_io *io,
                   const struct orlg_step_diag *diag) {
    return step_entry(e, ORLG_ENTRY_PLAIN, policy, 0, 0, n_steps, actions, auto_reset, io, step_extras(diag));
}
int orlg_step_gn_protect(orlg_env *e, int32_t policy, int32_t n_steps, const int32_t *actions, int32_t auto_reset, const orlg_step_io *io,
                         const struct orlg_step_diag *diag, double *gn_neighbour_margin_db) {
    return step_entry(e, ORLG_ENTRY_PLAIN, policy, 0, 0, n_steps, actions, auto_reset, io, step_extras(diag, gn_neighbour_margin_db));
}
int orlg_step_assign(orlg_env *e, int32_t policy, int32_t assign, int32_t n_steps, const int32_t *actions, int32_t auto_reset,
                     const orlg_step_io *io, const struct orlg_step_diag *diag) {
    return step_entry(e, ORLG_ENTRY_ASSIGN, policy, assign, 0, n_steps, actions, auto_reset, io, step_extras(diag));
}
int orlg_step_min_cut(orlg_env *e, int32_t route, int32_t n_steps, const int32_t *actions, int32_t auto_reset, const orlg_step_io *io,
                      const struct orlg_step_diag *diag) {
    return step_entry(e, ORLG_ENTRY_MIN_CUT, route, 0, 0, n_steps, actions, auto_reset, io, step_extras(diag));
}
int orlg_step_window(orlg_env *e, int32_t route, int32_t rule, int32_t n_steps, const int32_t *actions, int32_t auto_reset, const orlg_step_io *io,
                     const struct orlg_step_diag *diag) {
    return step_entry(e, ORLG_ENTRY_WINDOW, route, rule, 0, n_steps, actions, auto_reset, io, step_extras(diag));
}
int orlg_step_rule_gn(orlg_env *e, int32_t route, int32_t rule, int32_t gn_mode, int32_t n_steps, const int32_t *actions, int32_t auto_reset,
                      const orlg_step_io *io, const struct orlg_step_diag *diag) {
    return step_entry(e, ORLG_ENTRY_RULE_GN, route, rule, gn_mode, n_steps, actions, auto_reset, io, step_extras(diag));
}
// a max-margin policy behind the gate: resolved by orlg_step_mm_call, one launch of orlg_rmsa_mm_kernel
int orlg_step_max_margin_protect(orlg_env *e, int32_t route, int32_t n_steps, const int32_t *actions, int32_t auto_reset, const orlg_step_io *io,
                                 const struct orlg_step_diag *diag, double *window_margin_db, double *gn_neighbour_margin_db) {
    if (!e) return fail(ORLG_ERR_INVALID, "null handle");
    if (e->p.gn_adaptive)
        return fail(ORLG_ERR_INVALID, "orlg_step_max_margin: the handle's gate chooses the modulation (orlg_set_gn_modulation), and no max-margin policy runs behind it yet");
    OrlgStepCall call;
    if (int rc = orlg_step_mm_call({route, n_steps, e->p.gn != nullptr, actions != nullptr}, &call)) return rc;
    WaveFamily mm;
    mm.family = ORLG_WAVE_MM;
    if (int rc = mm_geometry(e, &mm.mm)) return rc;
    StepExtras x = step_extras(diag, gn_neighbour_margin_db);
    x.wmargin = window_margin_db;
    return rmsa_step(e, call, n_steps, actions, auto_reset, io, x, mm);
}
int orlg_step_max_margin(orlg_env *e, int32_t route, int32_t n_steps, const int32_t *actions, int32_t auto_reset, const orlg_step_io *io,
                         const struct orlg_step_diag *diag, double *window_margin_db) {
    return orlg_step_max_margin_protect(e, route, n_steps, actions, auto_reset, io, diag, window_margin_db, nullptr);
}
// a policy that walks the levels behind a gate that chooses the modulation: one launch of orlg_rmsa_am_kernel
int orlg_step_modulation(orlg_env *e, int32_t policy, int32_t n_steps, const int32_t *actions, int32_t auto_reset, const orlg_step_io *io,
                         double *gn_gsnr_db, uint8_t *gn_se) {
    if (!e) return fail(ORLG_ERR_INVALID, "null handle");
    if (!e->p.gn || !e->p.gn_adaptive)
        return fail(ORLG_ERR_INVALID, "orlg_step_modulation: the handle's gate does not choose the modulation (orlg_set_gn_modulation with ORLG_GN_MODULATION_ADAPTIVE on a handle with a gn_gate)");
    if (policy < ORLG_AM_SP_FF || policy > ORLG_AM_EXTERNAL)
        return fail(ORLG_ERR_INVALID, "orlg_step_modulation needs a policy ORLG_AM_SP_FF .. ORLG_AM_EXTERNAL: got %d", policy);
    if (n_steps < 1) return fail(ORLG_ERR_INVALID, "n_steps must be >= 1");
    const OrlgStepCall call = {(int32_t)ORLG_POLICY_SP_AM + (policy - ORLG_AM_SP_FF), ORLG_ASSIGN_FIRST};
    StepExtras x;
    x.gsnr = gn_gsnr_db;
    x.se = gn_se;
    WaveFamily am;
    am.family = ORLG_WAVE_AM;
    return rmsa_step(e, call, n_steps, actions, auto_reset, io, x, am);
}
}  // extern "C"

// ---------------------------------------------------------------------------------------- the gate
int gn_gate_table(const orlg_env *e, const orlg_rmsa_gn_gate *g, std::vector<double> &tab) {
    const int E = e->p.E;
    if (!g->link_num_spans || !g->link_span_length_km || !g->thresholds_db) return fail(ORLG_ERR_INVALID, "null argument");
    const struct { const char *name; double v; } scalars[] = {
        {"launch_power_density_w_hz", g->launch_power_density_w_hz}, {"frequency_start_hz", g->frequency_start_hz},
        {"slot_width_hz", g->slot_width_hz}, {"attenuation_normalized", g->attenuation_normalized}, {"noise_figure", g->noise_figure}};
    for (const auto &sc : scalars)
        if (!std::isfinite(sc.v) || !(sc.v > 0)) return fail(ORLG_ERR_INVALID, "gn_gate: %s must be finite and positive", sc.name);
    if (g->num_thresholds < 1 || g->num_thresholds > ORLG_GN_LINK0 - ORLG_GN_THR0)
        return fail(ORLG_ERR_INVALID, "gn_gate: num_thresholds %d not in 1..%d", g->num_thresholds, ORLG_GN_LINK0 - ORLG_GN_THR0);
    for (int i = 0; i < g->num_thresholds; i++)
        if (!std::isfinite(g->thresholds_db[i])) return fail(ORLG_ERR_INVALID, "gn_gate: thresholds_db[%d] is not finite", i);
    for (size_t gid = 0; gid < e->path_se.size(); gid++) {
        if (e->path_se[gid] > g->num_thresholds)
            return fail(ORLG_ERR_INVALID, "gn_gate: path %zu has spectral efficiency %d, thresholds_db has %d entries", gid, e->path_se[gid], g->num_thresholds);
        if (e->path_se[gid] > 6)
            return fail(ORLG_ERR_INVALID, "gn_gate: path %zu has spectral efficiency %d, the modulation factors of the GN model end at 6", gid, e->path_se[gid]);
    }
    tab.assign(ORLG_GN_LINK0 + 4 * (size_t)E, 0.0);
    const double att = g->attenuation_normalized;
    tab[ORLG_GN_DENSITY] = g->launch_power_density_w_hz; tab[ORLG_GN_F0] = g->frequency_start_hz; tab[ORLG_GN_SLOT] = g->slot_width_hz;
    tab[ORLG_GN_ATT] = att; tab[ORLG_GN_NF] = g->noise_figure; tab[ORLG_GN_LEFF_A] = 1 / (2 * att);
    for (int i = 0; i < g->num_thresholds; i++) tab[ORLG_GN_THR0 + i] = g->thresholds_db[i];
    for (int l = 0; l < E; l++) {
        const double len = g->link_span_length_km[l];
        if (g->link_num_spans[l] < 1) return fail(ORLG_ERR_INVALID, "gn_gate: link_num_spans[%d] = %d", l, g->link_num_spans[l]);
        if (!std::isfinite(len) || !(len > 0)) return fail(ORLG_ERR_INVALID, "gn_gate: link_span_length_km[%d] must be finite and positive", l);
        // per span, as calculate_osnr.py:24-26, 50 writes them
        const double l_eff = (1 - std::exp(-2 * att * len * 1e3)) / (2 * att);
        const double e1 = std::exp(2 * att * len * 1e3) - 1;
        if (!std::isfinite(e1)) return fail(ORLG_ERR_INVALID, "gn_gate: the loss of a span of link %d overflows", l);
        double *row = &tab[ORLG_GN_LINK0 + 4 * (size_t)l];
        row[0] = l_eff; row[1] = l_eff / (len * 1e3); row[2] = e1; row[3] = (double)g->link_num_spans[l];
    }
    return ORLG_OK;
}

extern "C" {
int orlg_set_gn_gate(orlg_env *e, const orlg_rmsa_gn_gate *g) {
    if (!e) return fail(ORLG_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(e->device));
    if (!g) {
        if (e->p.gn_adaptive)
            return fail(ORLG_ERR_INVALID, "gn_gate: the handle's gate chooses the modulation (orlg_set_gn_modulation): its running services carry levels that no handle without a gate can read");
        e->p.gn = nullptr;
        e->gn_protect = false;   // (protection is a property of the gate: a new gate keeps it, no gate has none)
        return ORLG_OK;
    }
    if (e->group_mode == ORLG_KERNEL_GROUP)
        return fail(ORLG_ERR_INVALID, "gn_gate: the admission check is served by the wave-per-environment kernel, the handle was created with step_kernel GROUP");
    if (e->p.gn_adaptive && g->num_thresholds != e->p.gn_adaptive)
        return fail(ORLG_ERR_INVALID, "gn_gate: the handle's gate chooses among %d levels (orlg_set_gn_modulation), the new gate has %d thresholds", e->p.gn_adaptive, g->num_thresholds);
    std::vector<double> tab;
    if (int rc = gn_gate_table(e, g, tab)) return rc;
    if (!e->gn_table)
        if (int rc = orlg_handle_alloc(e, &e->gn_table, tab.size())) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));   // (a launch in flight may be reading the table)
    HIP_TRY(hipMemcpy(e->gn_table, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    e->p.gn = e->gn_table;
    e->gn_num_thresholds = g->num_thresholds;
    return ORLG_OK;
}

int orlg_set_gn_protect(orlg_env *e, int32_t on) {
    if (!e) return fail(ORLG_ERR_INVALID, "null handle");
    if (!e->p.gn) return fail(ORLG_ERR_INVALID, "gn_protect: the handle has no gn_gate (orlg_set_gn_gate): protection is a property of the gate");
    if (on && e->p.gn_adaptive)
        return fail(ORLG_ERR_INVALID, "gn_protect: the handle's gate chooses the modulation (orlg_set_gn_modulation), and the running lightpaths are not protected behind it yet");
    e->gn_protect = on != 0;
    return ORLG_OK;
}

int orlg_set_gn_modulation(orlg_env *e, int32_t mode) {
    if (!e) return fail(ORLG_ERR_INVALID, "null handle");
    if (!e->p.gn) return fail(ORLG_ERR_INVALID, "gn_modulation: the handle has no gn_gate (orlg_set_gn_gate): the mode is a property of the gate");
    if (mode != ORLG_GN_MODULATION_PATH && mode != ORLG_GN_MODULATION_ADAPTIVE)
        return fail(ORLG_ERR_INVALID, "gn_modulation: unknown mode %d (ORLG_GN_MODULATION_PATH or ORLG_GN_MODULATION_ADAPTIVE)", mode);
    HIP_TRY(hipSetDevice(e->device));
    if (mode == ORLG_GN_MODULATION_PATH) {
        if (e->p.gn_adaptive) {   // (the levels its services carry would read as path records)
            HIP_TRY(hipStreamSynchronize(e->stream));
            const int has = rmsa_state_has_levels(e, e->p.qdesc);
            if (has < 0) return has;
            if (has) return fail(ORLG_ERR_INVALID, "gn_modulation: the state holds a service that runs at a level of its own; a gate that does not choose the modulation cannot read it");
        }
        e->p.gn_adaptive = 0;
        return ORLG_OK;
    }
    if (e->gn_protect)
        return fail(ORLG_ERR_INVALID, "gn_modulation: the handle protects its running lightpaths (orlg_set_gn_protect), and the modulation is not chosen behind that second check yet");
    if (e->num_paths >= ORLG_QDESC_AM_PATHS)
        return fail(ORLG_ERR_INVALID, "gn_modulation: %d path records; a service's level takes 3 bits of the descriptor's path field, which leaves room for %d", e->num_paths, ORLG_QDESC_AM_PATHS - 1);
    const int M = e->gn_num_thresholds;
    if (M < 1 || M > ORLG_QDESC_MAX_LEVEL)
        return fail(ORLG_ERR_INVALID, "gn_modulation: the gate has %d thresholds; the levels are spectral efficiencies 1..%d, where the modulation factors of the GN model end", M, ORLG_QDESC_MAX_LEVEL);
    e->p.gn_adaptive = M;
    return ORLG_OK;
}

}  // extern "C"
