// orlg_gn_audit_kernels.hip -- the GN-model audit of every running lightpath of every environment, and the list of the running
// services it audits (include/orlg.h orlg_gn_audit, orlg_get_running_services).  A unit of its own and ONE object:
// nothing here depends on the word count W (no occupancy row is read), so it needs no orlg_inst_* object per W.
//
// orlg_gn_audit_kernel has the shape of orlg_gn_action_masks_kernel: tables staged once per workgroup, one wave per environment at
// a time, the grid sized to the device and striding over the batch, the LIVE descriptors of the release ring copied to LDS in rank
// order (n_running entries from q_head to positions 0 .. n), so that the walk never meets a wrap.  Then a wave-uniform loop over
// the victims, rmsa_gn_audit_victim (orlg_rmsa_gn_audit.h) each.  Where the ring fits one chunk (n <= 64) every lane decodes its
// entry once per environment and keeps it for the whole loop.  The per-service values collect on lane = rank % 64 and leave 64 at a
// time; the summary comes from a wave minimum.  The release times are not needed: a state between launches holds no service that
// is due at the pending request's arrival.  Both kernels read state and write only the caller's buffers.
#include "../../include/orlg.h"
#include "orlg_rmsa_gn_audit.h"
#include "orlg_variants.h"

#define ORLG_AUDIT_NAN __longlong_as_double(0x7ff8000000000000ll)

// n_running and q_head of an environment as every reader of the ring clamps them (n_running also counts services an overflow lost)
DEV void audit_ring(const OrlgEnvScalars *sc, int Q, int &head, int &n) {
    const int q_head = uni(sc->q_head), n_run = uni(sc->n_running);
    head = q_head >= 0 && q_head < Q ? q_head : 0;
    n = n_run < Q ? (n_run < 0 ? 0 : n_run) : Q;
}

// summary: [B]; gsnr, margin, ase, nli: [B][Q] doubles in rank order, NaN past n; any of them may be nullptr.  `table`: the gate's
// table (ORLG_GN_*), the handle's own or one built for this call.  LDS per wave: Q descriptors.
__global__ __launch_bounds__(ORLG_WAVE *ORLG_MAX_WAVES_PER_BLOCK) void orlg_gn_audit_kernel(const OrlgParams p, const double *table,
                                                                                            orlg_gn_audit_summary *summary, double *gsnr,
                                                                                            double *margin, double *ase, double *nli) {
    extern __shared__ __align__(16) unsigned char smem[];
    stage_tables(smem, p);
    const Tab tb = make_tab(smem, p);
    const int lane = threadIdx.x & 63;
    const int wib = uni((int)(threadIdx.x >> 6));
    const int Q = p.Q, q_bytes = (Q * 4 + 15) & ~15;
    Wave wv = {};
    wv.lane = lane;
    wv.qdesc = reinterpret_cast<uint32_t *>(smem + p.l_shared_bytes + (size_t)wib * q_bytes);
    const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
    const OrlgGnTable gn = ORLG_GPTR(const double, table);
    const bool wide = p.E > 64;
    const bool services = gsnr || margin || ase || nli;
    const bool adaptive = p.gn_adaptive != 0;   // the descriptors carry the level their service runs at (orlg_qdesc.h)
    const double nan = ORLG_AUDIT_NAN, inf = __longlong_as_double((long long)ORLG_INF_BITS);
    for (int env = blockIdx.x * (int)(blockDim.x >> 6) + wib; env < p.B; env += n_waves) {
        int q_head, q_n;
        audit_ring(p.scal + env, Q, q_head, q_n);
        {
            const uint32_t *g = p.qdesc + (size_t)env * Q;
            for (int i = lane; i < q_n; i += 64) {
                int pos = q_head + i;
                pos -= pos >= Q ? Q : 0;
                wv.qdesc[i] = g[pos];
            }
        }
        wave_sync();
        const bool resident = q_n <= 64;
        OrlgGnAuditEntry mine = {};
        if (resident && q_n > 0) mine = rmsa_gn_audit_decode(tb, gn, wv.qdesc[lane < q_n ? lane : 0], wide, adaptive);
        const size_t row = (size_t)env * Q;
        double c_g = nan, c_m = nan, c_a = nan, c_n = nan;   // lane r: the values of rank (v & ~63) + r
        double my_min = inf;                                // ... the smallest margin of the ranks this lane took, its lowest rank
        int my_rank = 0x7fffffff, my_below = 0;
        for (int v = 0; v < q_n; ++v) {
            const OrlgGnAuditValue r = rmsa_gn_audit_victim(wv, tb, gn, wide, q_n, v, resident, mine, adaptive);
            // (every service is audited at the threshold of the level it runs at)
            const int se = orlg_qdesc_se(orlg_qdesc_level(wv.qdesc[v], adaptive), (int)tb.recs[orlg_qdesc_gid(wv.qdesc[v], adaptive)].se);
            const double m = r.gsnr_db - gn[ORLG_GN_THR0 + se - 1];
            if (lane == (v & 63)) {
                c_g = r.gsnr_db; c_m = m; c_a = r.ase_db; c_n = r.nli_db;
                my_below += m < 0 ? 1 : 0;
                if (m < my_min) { my_min = m; my_rank = v; }
            }
            if (services && ((v & 63) == 63 || v == q_n - 1)) {
                const int at = (v & ~63) + lane;
                if (at <= v) {
                    if (gsnr) gsnr[row + at] = c_g;
                    if (margin) margin[row + at] = c_m;
                    if (ase) ase[row + at] = c_a;
                    if (nli) nli[row + at] = c_n;
                }
            }
        }
        if (services)
            for (int i = q_n + lane; i < Q; i += 64) {
                if (gsnr) gsnr[row + i] = nan;
                if (margin) margin[row + i] = nan;
                if (ase) ase[row + i] = nan;
                if (nli) nli[row + i] = nan;
            }
        if (summary) {
            // the lowest rank that attains the minimum; its lane's value is the minimum, bit for bit.  A margin that is NaN (a
            // service whose sums left the logarithm's domain) is below no bound and attains no minimum
            const double lo = -wave_max_f64(-my_min);
            const int worst = wave_min_i32(my_min == lo && my_rank != 0x7fffffff ? my_rank : 0x7fffffff);
            const int below = wave_add_i32(my_below);
            const bool any = worst != 0x7fffffff;
            const double min_margin = any ? readlane_d(my_min, worst & 63) : nan;
            if (lane == 0) {
                orlg_gn_audit_summary *s = summary + env;
                s->n_running = q_n; s->n_below = below; s->worst_rank = any ? worst : -1; s->pad = 0;
                s->min_margin_db = min_margin;
            }
        }
        wave_sync();
    }
}

// the running services of every environment, decoded as the step decodes them: count, head [B]; the rest [B][Q] in rank order, -1 /
// NaN past count; any of them may be nullptr.  One thread per (environment, rank); the tables are read where they lie in HBM.
// se: the spectral efficiency the service runs at -- the level an adaptive handle stored with it (orlg_qdesc.h), else its path's own.
__global__ __launch_bounds__(256) void orlg_running_services_kernel(const OrlgParams p, int32_t *count, int32_t *head, int32_t *path_gid,
                                                                    int16_t *slot, int16_t *num_slots, int32_t *bit_rate,
                                                                    double *release_time, int16_t *se) {
    const OrlgPathRec *recs = reinterpret_cast<const OrlgPathRec *>(p.tables + p.t_recs);
    const uint16_t *nslots = reinterpret_cast<const uint16_t *>(p.tables + p.t_nslots);
    const int32_t *bit_rates = reinterpret_cast<const int32_t *>(p.tables + p.t_bitrates);
    const int Q = p.Q;
    const size_t total = (size_t)p.B * Q;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int env = (int)(i / Q), rank = (int)(i - (size_t)env * Q);
        const OrlgEnvScalars *sc = p.scal + env;
        const int q_head = sc->q_head, n_run = sc->n_running;
        const int h = q_head >= 0 && q_head < Q ? q_head : 0;
        const int n = n_run < Q ? (n_run < 0 ? 0 : n_run) : Q;
        if (rank == 0) {
            if (count) count[env] = n;
            if (head) head[env] = h;
        }
        int32_t gid = -1, br = -1;
        int16_t s = -1, ns = -1, lv = -1;
        double t = ORLG_AUDIT_NAN;
        if (rank < n) {
            int pos = h + rank;
            pos -= pos >= Q ? Q : 0;
            const uint32_t d = p.qdesc[(size_t)env * Q + pos];
            const bool adaptive = p.gn_adaptive != 0;
            gid = (int32_t)orlg_qdesc_gid(d, adaptive);
            s = (int16_t)((d >> 14) & 0x3ffu);
            lv = (int16_t)orlg_qdesc_se(orlg_qdesc_level(d, adaptive), (int)recs[gid].se);
            ns = (int16_t)nslots[(d >> 24) * ORLG_NSLOT_STRIDE + lv];
            br = bit_rates[d >> 24];
            t = p.qtime[(size_t)env * Q + pos];
        }
        if (path_gid) path_gid[i] = gid;
        if (slot) slot[i] = s;
        if (num_slots) num_slots[i] = ns;
        if (bit_rate) bit_rate[i] = br;
        if (release_time) release_time[i] = t;
        if (se) se[i] = lv;
    }
}

orlg_gn_audit_kernel_t orlg_gn_audit_kernel_lookup() { return orlg_gn_audit_kernel; }
orlg_running_services_kernel_t orlg_running_services_kernel_lookup() { return orlg_running_services_kernel; }
