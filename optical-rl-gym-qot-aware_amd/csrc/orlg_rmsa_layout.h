// orlg_rmsa_layout.h -- what the kernels of the RMSA / DeepRMSA path know about where an environment lies on chip.
//
// Tab: the read-only topology tables a workgroup stages into LDS (make_tab, stage_tables); Wave: one wave's environment in LDS
// (the wave-per-environment step kernel, orlg_kernels.hip); copy_words: the bulk copy between an environment's HBM arrays and
// LDS; apply_window: a slot window set or cleared on every link of a path in the wave's bitmap (it lives here and not in
// orlg_spectrum.h because it takes a Wave, and the QoT-aware kernels include orlg_spectrum.h); KernargParams / kernarg_params:
// the opaque re-read of OrlgParams from the kernarg segment.  The byte offsets themselves are OrlgParams' (orlg_device.h), computed
// by the host (rmsa_create, orlg_api.hip).
//
// Reference: optical_rl_gym/envs/rmsa_env.py _provision_path :462-513 and _release_path :515-535 (apply_window: the slot
// window of a service on the links of its path).
#pragma once
#include "orlg_wave.h"

// ---------------------------------------------------------------------------------------- contexts
struct Tab {  // topology tables staged in LDS (shared by the waves of a workgroup, read-only)
    const int32_t *pair_base;
    const OrlgPathRec *recs;
    const uint16_t *nslots;
    const int32_t *bit_rates;
    const double *br_cum, *src_cum, *dst_cum;
    const double *div_s, *inv_k;   // k / S and 1 / k tables (full statistics)
    const u64 *outs;
};

struct Wave {  // this wave's environment in LDS
    int lane;
    u64 *occ;
    double *qtime;
    uint32_t *qdesc;
    uint32_t *mt;
    double *lst;   // [4][E]
    int32_t *hist; // [4][NBR]
    int32_t *lint; // [E] span | gaps << 16
    uint32_t *scratch;
    OrlgWaveScalars *wsc;
    double *ring_iat, *ring_ht;  // [ORLG_RING] pre-generated arrivals
    uint32_t *ring_req;          // [ORLG_RING]
};

DEV Tab make_tab(unsigned char *smem, const OrlgParams &p) {
    Tab tb;
    tb.pair_base = reinterpret_cast<const int32_t *>(smem + p.t_pair);
    tb.recs = reinterpret_cast<const OrlgPathRec *>(smem + p.t_recs);
    tb.nslots = reinterpret_cast<const uint16_t *>(smem + p.t_nslots);
    tb.bit_rates = reinterpret_cast<const int32_t *>(smem + p.t_bitrates);
    tb.br_cum = reinterpret_cast<const double *>(smem + p.t_brcum);
    tb.src_cum = reinterpret_cast<const double *>(smem + p.t_srccum);
    tb.dst_cum = reinterpret_cast<const double *>(smem + p.t_dstcum);
    tb.div_s = reinterpret_cast<const double *>(smem + p.t_divs);
    tb.inv_k = reinterpret_cast<const double *>(smem + p.t_inv);
    tb.outs = reinterpret_cast<const u64 *>(smem + p.l_outs);
    return tb;
}

// stage the table blob (and the per-call output pointers) into LDS; every thread of the workgroup takes part
DEV void stage_tables(unsigned char *smem, const OrlgParams &p) {
    const uint4 *src = reinterpret_cast<const uint4 *>(p.tables);
    uint4 *dst = reinterpret_cast<uint4 *>(smem);
    const int n16 = p.tab_bytes >> 4;
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
#pragma unroll
    for (int i = 0; i < ORLG_NUM_OUTS; ++i)
        if ((int)threadIdx.x == i) reinterpret_cast<u64 *>(smem + p.l_outs)[i] = reinterpret_cast<u64>(p.outs[i]);
    __syncthreads();
}

// bulk copies between an environment's HBM arrays and the wave's LDS region: 16 bytes per lane per instruction (both sides
// are 16-byte aligned: LDS offsets by construction, HBM per-env strides checked by the caller), 4-byte tail
DEV void copy_words(void *dst, const void *src, int bytes, int lane) {
    const int n16 = bytes >> 4;
    const uint4 *s16 = reinterpret_cast<const uint4 *>(src);
    uint4 *d16 = reinterpret_cast<uint4 *>(dst);
    for (int i = lane; i < n16; i += 64) d16[i] = s16[i];
    const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src);
    uint32_t *d4 = reinterpret_cast<uint32_t *>(dst);
    for (int i = (n16 << 2) + lane; i < (bytes >> 2); i += 64) d4[i] = s4[i];
}

// set (release) or clear (provision) the window [s, s+n) on every link of a path
template <int W>
DEV void apply_window(Wave &wv, const uint8_t *links, int hops, int s, int n, bool set_free) {
    constexpr int HPC = 64 / W;
    const int hl = wv.lane / W, w = wv.lane - hl * W;
    u64 m = window_mask(s, n, w);
    for (int h0 = 0; h0 < hops; h0 += HPC) {
        int h = h0 + hl;
        if (hl < HPC && h < hops && m) {
            u64 *word = wv.occ + __mul24((int)links[h], W) + w;
            *word = set_free ? (*word | m) : (*word & ~m);
        }
    }
    wave_sync();
}

// the RMSA kernels re-read their parameters through an OPAQUE pointer: lets the compiler drop rarely used pointers from SGPRs
// across the step loop instead of spilling them
typedef const OrlgParams __attribute__((address_space(4))) *KernargParams;
DEV KernargParams kernarg_params() {
    auto k = kernarg_as<OrlgParams>();
    asm volatile("" : "+s"(k));
    return k;
}
