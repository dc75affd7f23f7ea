// orlg_phy_virtual.h -- the virtual layer and the release queue of the QoT-aware step kernel (orlg_phy_kernels.hip).
//
// Reference: optical_rl_gym/envs/phy_rmsa_env.py -- channel_state lists as _provision_virtual_path :625-659, _provision_path
// :600-602 and _release_path :781-861 rewrite them (CsList; the float64 shares of bit_rate_selection="continuous": CsShares);
// the release loop of _next_service :1009-1017 on a near-term buffer in LDS (NearBuffer, nb_rebuild, nb_first_due) with the
// next step's release looked up ahead (ReleaseAhead); a new service's record and its side arrays (rec_store, svc_side_store).
#pragma once
#include "orlg_phy_layout.h"
#include "orlg_requests.h"   // orlg_env_rates

// ---- channel_state lists (virtual layer): one list = up to cs_len packed entries, entry i on lane i
struct CsList { uint32_t e; int n, cap; };
DEV CsList cs_load(const uint32_t *cs, const uint8_t *cs_n, int key, int lane, int cs_len) {
    CsList l;
    l.n = uni((int)cs_n[key]);
    l.cap = cs_len;
    l.e = lane < l.n ? cs[(size_t)key * cs_len + lane] : 0u;
    return l;
}
DEV void cs_store(uint32_t *cs, uint8_t *cs_n, int key, const CsList &l, int lane) {
    if (lane < l.n) cs[(size_t)key * l.cap + lane] = l.e;
    if (lane == 0) cs_n[key] = (uint8_t)l.n;
}
DEV int cs_find(const CsList &l, int ch, int lane) {  // first entry with this channel number, -1 if none
    u64 m = ballot(lane < l.n && cs_ch(l.e) == ch);
    return m ? ctz64(m) : -1;
}
DEV uint32_t cs_get(const CsList &l, int q) { return (uint32_t)__builtin_amdgcn_readlane((int)l.e, q); }
DEV void cs_remove(CsList &l, int q, int lane) {  // list.remove(entry q): later entries move up
    uint32_t nxt = (uint32_t)__shfl_down((int)l.e, 1);
    if (lane >= q) l.e = lane + 1 < l.n ? nxt : 0u;
    l.n -= 1;
}
DEV bool cs_append(CsList &l, uint32_t v, int lane) {  // list.append
    if (l.n >= l.cap) return false;
    if (lane == l.n) l.e = v;
    l.n += 1;
    return true;
}
// continuous bit rates: the float64 (used, free) of a list's entries, lane i = entry i next to CsList::e (whose used / free
// fields stay 0: channel, capacity and the valid bit are all the packed word keeps).  Every csf_* call comes before the
// cs_* call it pairs with (they take the list length as it was).
struct CsShares { double u, f; };
DEV CsShares csf_load(const double *csf, int key, int lane, int n, int cs_len) {
    CsShares s;
    s.u = 0.0; s.f = 0.0;
    if (lane < n) {
        const double *q = csf + ((size_t)key * cs_len + lane) * 2;
        s.u = q[0]; s.f = q[1];
    }
    return s;
}
DEV void csf_store(double *csf, int key, const CsShares &s, int n, int cs_len, int lane) {
    if (lane < n) {
        double *q = csf + ((size_t)key * cs_len + lane) * 2;
        q[0] = s.u; q[1] = s.f;
    }
}
DEV void csf_remove(CsShares &s, int q, int n, int lane) {
    const double nu = __shfl_down(s.u, 1), nf = __shfl_down(s.f, 1);
    if (lane >= q) {
        s.u = lane + 1 < n ? nu : 0.0;
        s.f = lane + 1 < n ? nf : 0.0;
    }
}
DEV void csf_append(CsShares &s, double u, double f, int n, int cap, int lane) {
    if (n < cap && lane == n) { s.u = u; s.f = f; }
}

// ---- near-term release buffer.  The release loop of _next_service (phy_rmsa_env.py:1009-1017) pops every event with
// time <= now; with ~load running services a scan of all release times per step would need them all in LDS.  Instead
// the LDS buffer holds (time, queue index) of every running service with release time <= horizon (it may hold a few
// later ones too); now <= horizon always holds when the loop looks for due services, so the buffer is all it has to
// read.  When the clock passes the horizon, or the buffer fills up, it is rebuilt from the HBM array with a horizon
// that is expected to catch half a buffer (exponential holding times: n_running * holding_lambda releases per unit time).
struct NearBuffer {
    double *t;        // [ORLG_PHY_NB] release times
    uint16_t *qi;     // [ORLG_PHY_NB] index of the service in the HBM queue
    int n;
    double horizon;
};
DEV int nb_collect(NearBuffer &nb, const double *gq, int n_running, double horizon, int lane) {
    int cnt = 0;
    for (int i0 = 0; i0 < n_running; i0 += 64) {
        const int i = i0 + lane;
        const double tq = i < n_running ? gq[i] : __longlong_as_double((long long)ORLG_INF_BITS);
        const bool in = tq <= horizon;
        const u64 m = ballot(in);
        if (m) {
            const int pos = cnt + popc64(m & ((1ull << lane) - 1ull));
            if (in && pos < ORLG_PHY_NB) { nb.t[pos] = tq; nb.qi[pos] = (uint16_t)i; }
            cnt += popc64(m);
        }
    }
    wave_sync();
    return cnt;
}
// the holding rate that sizes the horizon of nb_rebuild: the handle's scalar, or the environment's own of a handle with
// per-environment traffic -- fetched from the kernel arguments and the scalar cache at the call, not kept in a register
DEV double phy_holding_lambda(double holding_lambda, int env) {
    const auto kq = kernarg_as<OrlgPhyParams>();
    double arrival_lambda = 0.0;
    orlg_env_rates(kq->rates, env, arrival_lambda, holding_lambda);
    return holding_lambda;
}
// returns false when even the services due right now do not fit (reported as a queue overflow)
DEV bool nb_rebuild(NearBuffer &nb, const double *gq, int n_running, double now, double holding_lambda, int lane) {
    double delta = (double)ORLG_PHY_NB / (2.0 * (double)(n_running > 0 ? n_running : 1) * holding_lambda);
    for (int it = 0; it < 48; ++it) {
        const double h = now + delta;
        const int cnt = nb_collect(nb, gq, n_running, h, lane);
        if (cnt <= ORLG_PHY_NB) { nb.n = cnt; nb.horizon = h; return true; }
        delta *= 0.5;
    }
    const int cnt = nb_collect(nb, gq, n_running, now, lane);
    nb.n = cnt <= ORLG_PHY_NB ? cnt : ORLG_PHY_NB;
    nb.horizon = now;
    return cnt <= ORLG_PHY_NB;
}

// ---- the release of the NEXT step, looked up ahead.  The arrival times come from the pre-generated ring, so the release
// loop's scan already knows the time of the following arrival and finds the service that will be released first then; its
// record is requested right away and is on lanes when the next step's release loop needs it.  That loop still finds its
// victims by itself: the record is used only when its first victim is the one looked up (anything else is a plain load).
// (Requesting the service's channel_state list, node weights and the queue's last record ahead as well was measured: no
// gain, four more registers held across the step.)
struct ReleaseAhead {
    int q;            // queue index of the looked-up service, -1: none
    uint32_t rec;     // lane < 12: dword `lane` of its record
};
DEV uint32_t rec_dword(const OrlgPhySvc *grec, int q, int lane) {
    return lane < 12 ? reinterpret_cast<const uint32_t *>(grec + q)[lane] : 0u;
}
static_assert(sizeof(OrlgPhySvc) == 48 && ORLG_PHY_MAX_CH == 14, "record = 12 dwords: arrival, seq, gid | nch | flags, 14 channels, pad");
// a new record written by lanes: lane i < nch holds channel i's halfword (0xffff beyond), dwords 4..10 pair them up
DEV uint32_t rec_store(OrlgPhySvc *dst, const double *arrival_lds, uint32_t seq, int gid, int nch, int flags, uint32_t hw, int lane) {
    const int j = lane >= 4 ? lane - 4 : 0;
    const uint32_t h0 = (uint32_t)__shfl((int)hw, 2 * j), h1 = (uint32_t)__shfl((int)hw, 2 * j + 1);
    uint32_t v = h0 | (h1 << 16);
    if (lane < 2) v = reinterpret_cast<const uint32_t *>(arrival_lds)[lane];
    if (lane == 2) v = seq;
    if (lane == 3) v = (uint32_t)gid | ((uint32_t)nch << 16) | ((uint32_t)flags << 24);
    if (lane == 11) v = 0u;
    if (lane < 12) reinterpret_cast<uint32_t *>(dst)[lane] = v;
    return v;
}
// the side arrays of a new record (OrlgPhyParams::qsum / qseq): hw = the halfword of channel `lane` as rec_store takes it
DEV void svc_side_store(u64 *gsum, uint32_t *gseq, int q, int gid, int flags, int nch, uint32_t hw, uint32_t seq, int lane) {
    const uint32_t h0 = (uint32_t)__builtin_amdgcn_readlane((int)hw, 0), h1 = (uint32_t)__builtin_amdgcn_readlane((int)hw, 1);
    if (lane == 0) {
        gsum[q] = svc_summary(gid, flags, nch, h0, nch > 1 ? h1 : 0u);
        gseq[q] = seq;
    }
}
// first service due at `time` among the near buffer's entries (earliest release, ties: lowest queue index)
DEV void nb_first_due(const NearBuffer &nb, double time, int lane, int &victim, int &vpos, double &best_t) {
    best_t = 0.0;
    victim = -1; vpos = -1;
    for (int c0 = 0; c0 < nb.n; c0 += 64) {
        const int c = c0 + lane;
        const double tq = c < nb.n ? nb.t[c] : __longlong_as_double((long long)ORLG_INF_BITS);
        const int qi = c < nb.n ? (int)nb.qi[c] : 0;
        u64 m = ballot(tq <= time);
        while (m) {
            const int l = ctz64(m);
            m &= m - 1;
            const double tt = readlane_d(tq, l);
            const int qq = __builtin_amdgcn_readlane(qi, l);
            if (victim < 0 || tt < best_t || (tt == best_t && qq < victim)) { best_t = tt; victim = qq; vpos = c0 + l; }
        }
    }
}
