// orlg_phy_layout.h -- data layout of the QoT-aware (PhyRMSA) path: what the step kernel (orlg_phy_kernels.hip) and the host side
// (orlg_phy_api.hip and its helper kernels) both have to know.
//
// The constants; a running service's record (OrlgPhySvc: service.channels of phy_rmsa_env.py:544-623), a defragmentation work
// list entry (OrlgPhyCand), the per-environment scalars in HBM (OrlgPhyScalars: the episode sums of phy_rmsa_env.py:103-112) and
// their LDS copy (PhyWaveScalars), the kernel arguments (OrlgPhyParams), the
// per-step outputs (ORLG_PHY_OUT_*); the packers of a channel_state tuple (cs_*: phy_rmsa_env.py:600-602, 640-644) and of a
// record's head (svc_summary / sum_*); the tables staged into LDS (PhyTab / make_phy_tab).
#pragma once
#include "orlg_wave.h"

#define ORLG_PHY_MAX_CH 14
#define ORLG_PHY_MAX_K 5
#define ORLG_PHY_NB 128   // entries of the near-term release buffer (LDS)
#define ORLG_RLOG_CAP 384  // entries of an environment's log of rewritten RSS terms (OrlgPhyParams::rlog_val / rlog_key)

struct __attribute__((aligned(16))) OrlgPhySvc {  // one running service (HBM)
    double arrival;                // service.arrival_time (age of a defragmentation candidate)
    uint32_t seq;                  // ascending seq = order of topology.graph["running_services"] (remove + append = new seq)
    uint16_t gid;
    uint8_t nch, flags;            // flags bit 0: served on the virtual layer; bit 1: source index > destination index
    uint16_t ch[ORLG_PHY_MAX_CH];  // service.channels in list order: channel | used << 9 | partial << 14  (partial: used != capacity)
};
// one entry of the per-env defragmentation work list (HBM): a candidate (diff, age, seq, idx, channel | position << 9)
// of the physical pass or a groom-eligible service (seq, idx) of the grooming pass
struct OrlgPhyCand { double diff, age; uint32_t seq; uint16_t idx, chj; uint16_t gid, pad0; uint32_t pad1; };
static_assert(sizeof(OrlgPhyCand) == 32, "OrlgPhyCand layout");
#define ORLG_CS_MAX 64             // entries per channel_state[src, dst, k-path] list: p.cs_len <= one wavefront
// one channel_state tuple (channel, used, free, capacity), 100 Gb/s units: ch | used << 9 | free << 14 | cap << 19 | 1 << 31
DEV uint32_t cs_pack(int ch, int used, int free_, int cap) {
    return (uint32_t)ch | ((uint32_t)used << 9) | ((uint32_t)free_ << 14) | ((uint32_t)cap << 19) | 0x80000000u;
}
DEV int cs_ch(uint32_t e) { return (int)(e & 0x1ffu); }
DEV int cs_used(uint32_t e) { return (int)((e >> 9) & 0x1fu); }
DEV int cs_free(uint32_t e) { return (int)((e >> 14) & 0x1fu); }
DEV int cs_cap(uint32_t e) { return (int)((e >> 19) & 0x1fu); }
static_assert(sizeof(OrlgPhySvc) == 48, "OrlgPhySvc layout");
// the head of a record in one 64-bit word (OrlgPhyParams::qsum): path, flags, channel count and the first two entries of
// service.channels (channel | used << 9 | partial << 14: 15 bits each; a service has 1.4 channels on average, the others are read
// from the record when nch > 2)
DEV u64 svc_summary(int gid, int flags, int nch, uint32_t hw0, uint32_t hw1) {
    return (u64)(uint32_t)gid | ((u64)(uint32_t)flags << 14) | ((u64)(uint32_t)nch << 16) | ((u64)(hw0 & 0x7fffu) << 20) | ((u64)(hw1 & 0x7fffu) << 35);
}
DEV int sum_gid(u64 s) { return (int)(s & 0x3fffu); }
DEV int sum_flags(u64 s) { return (int)((s >> 14) & 3u); }
DEV int sum_nch(u64 s) { return (int)((s >> 16) & 15u); }
DEV int sum_ch(u64 s, int j) { return (int)((s >> (20 + 15 * j)) & 0x7fffu); }   // j = 0, 1

// per-env scalars in HBM (256 B)
struct __attribute__((aligned(16))) OrlgPhyScalars {
    double current_time, req_arrival, req_holding;
    double total_path_length, total_gsnr;        // per-episode sums (phy_rmsa_env.py:103-105)
    int64_t c[8];                                // orlg_counters order
    int64_t total_path_index, total_mod, channels_accepted, physical_accepted;
    int64_t episodes_done;
    int32_t n_running, req_src, req_dst, req_br, req_sid, mt_idx, new_service, q_overflow;
    int32_t next_seq, counted_moves, counted_moves_groom, counted_defrag_cycles;  // phy_rmsa_env.py:110-112
    int32_t ring_pos, ring_cnt;                  // pre-generated arrivals: next entry, entries left (OrlgPhyParams::ring_*)
    int32_t pad[4];                              // pad[0]: the handle's channel count, stamped by the host when it clears the
                                                 // state (orlg_phy_api.hip); the step kernel never writes the padding
};
static_assert(sizeof(OrlgPhyScalars) == 224, "OrlgPhyScalars layout");

// policies: ORLG_PHY_POLICY_* of include/orlg.h
enum { ORLG_PHY_OUT_PATH = 0, ORLG_PHY_OUT_NCH, ORLG_PHY_OUT_CHANNELS, ORLG_PHY_OUT_ACCEPTED, ORLG_PHY_OUT_DONE,
       ORLG_PHY_OUT_REQUEST, ORLG_PHY_OUT_ARRIVAL, ORLG_PHY_OUT_HOLDING, ORLG_PHY_OUT_CUTS, ORLG_PHY_OUT_RSS,
       ORLG_PHY_OUT_CH_USED, ORLG_PHY_OUT_DEFRAG, ORLG_PHY_OUT_GN, ORLG_PHY_NUM_OUTS };

struct OrlgPhyParams {
    int32_t B, N, E, C, K, NBR, Q, NW;
    int32_t episode_length, n_steps, policy, auto_reset, mode, out_mask, num_rows, cpad;
    int32_t grooming, cs_len;
    int32_t defrag_period, number_moves, defrag_metric /* 0 cut, 1 rss */, cand_cap;
    double arrival_lambda, holding_lambda;
    // per-env state in HBM
    uint64_t *occ;          // [B][E*W]
    double *qtime;          // [B][Q]   release times, compact: entries 0..n_running-1 are live
    OrlgPhySvc *qrec;       // [B][Q]
    uint32_t *mt;           // [B][624] MT19937 state: fetched only when an environment's arrival ring runs dry
    double *ring_iat, *ring_ht;   // [B][64] pre-generated inter-arrival / holding times, in RNG stream order (refill_requests)
    uint32_t *ring_req;           // [B][64] src | dst << 8 | bit-rate index << 16
    OrlgPhyScalars *scal;   // [B]
    uint32_t *cs;           // [B][N*N*K][cs_len] channel_state lists (virtual layer), list order = array order
    uint8_t *cs_n;          // [B][N*N*K] list lengths
    // bit_rate_selection="continuous" (the CONT instantiations) shares the fields of the periodic defragmentation, which such a
    // handle does not have (refused at create time): the discrete kernels' arguments keep their layout, and so their code.
    // The bit rate is br_lower + r (r: the ring entry's draw); channel shares are float64 (phy_rmsa_env.py:1305-1308, 1666-1670,
    // 823-838) in arrays parallel to the packed channel_state entries and service records
    union {
        OrlgPhyCand *cand;      // [B][cand_cap] defragmentation work list (only with defrag_period > 0)
        double *out_share;      // CONT: per-step output [n_steps][B][ORLG_PHY_MAX_CH][2] the chosen channels' (used, free), or nullptr
    };
    // side arrays of the service records for the periodic defragmentation (only with defrag_period > 0, kept by the DF
    // instantiations at every site that writes a record): its scans walk 8 + 4 bytes per running service instead of 48
    union {
        uint64_t *qsum;     // [B][Q] svc_summary: gid | flags << 14 | nch << 16 | ch[0] << 20 | ch[1] << 35 (15-bit channel entries)
        double *cs_f;       // CONT: [B][N*N*K][cs_len][2] (used, free) of every channel_state entry, parallel to cs
    };
    union {
        uint32_t *qseq;     // [B][Q] the record's seq (list order of topology.graph["running_services"])
        double *svc_f;      // CONT: [B][Q][ORLG_PHY_MAX_CH] service.channels[i][1] (used), parallel to qrec
    };
    union {
        const uint64_t *lvl_mask;   // [num_rows*K][32][W] channels of one modulation level on (table row, k-path), as bit masks
        const double *act_share;    // CONT, external actions: [B][ORLG_PHY_MAX_CH][2] (used, free) of every chosen channel
    };
    uint32_t *ticket;       // work queue counter; environment = ticket - ticket_base
    uint32_t ticket_base, ticket_stride;
    // shared tables
    const unsigned char *tables;   // blob staged into LDS
    int32_t tab_bytes, t_pair, t_recs, t_bitrates, t_brcum, t_srccum, t_dstcum, t_pairrow, t_adjoff, t_adj, t_sqrt,
        t_plen, t_pathpair, t_masks;
    int32_t use_masks, br_lower;    // E <= 32: link sets as 32-bit masks (OrlgPathMasks) instead of the adjacency CSR; CONT: lower bound
    // cut metric through per-node free degrees (orlg_phy_config::path_node_weights), networks of at most 16 nodes of at most
    // 15 links each: D[channel] = 16 nibbles (nibble v = links at node v that are free on the channel) in the wave's LDS next
    // to the occupancy (l_nv), rebuilt from the occupancy at the start of every launch that evaluates the cut metric
    const uint4 *nvrec;     // [num_paths][2] node weights c (16 bytes: even nodes, then odd nodes) | wsum, cq (int16), chords
    int32_t use_nv;         // this launch keeps D (the handle has the tables and the launch's policy / defragmentation use the cut metric)
    int32_t l_nv, t_lnib, pad_nv;   // per-wave LDS offset of D; table: per link, 1 in the nibbles of its two end nodes
    // GN-model admission check of the chosen channels (include/orlg.h orlg_gn_gate), gn_on = 0: off
    int32_t gn_on, gn_nthr;
    double gn_pw, gn_bw, gn_att, gn_nf;
    const double *gn_cf;        // [C] centre frequencies
    const int32_t *gn_nspans;   // [E]
    const double *gn_spanlen;   // [E] km
    const double *gn_thr;       // [gn_nthr] dB, ascending
    // what the check evaluates that depends on the tables only, built once per handle ON THE DEVICE by orlg_gn_tables_kernel
    // with the very expressions gn_gsnr used to evaluate per check (same compiler, same libm routines: the same bits)
    const double *gn_A;         // [C][cpad] asinh(k (f_c - f_ch + bw/2)) - asinh(k (f_c - f_ch - bw/2)), 0 on the diagonal
    const double *gn_R;         // [C][cpad] bw / |f_c - f_ch|, 0 on the diagonal
    const double *gn_link;      // [E][4] l_eff, l_eff / span length, exp(2 att len) - 1, -; then [4E] = the self-channel asinh term
    // the channel-order sums of rss_total_metric, deferred (mc_flush): per env the terms at the start of a block of steps [cpad]
    // and the block's log of rewritten terms (value; channel | stamp << 16) [ORLG_RLOG_CAP each]
    double *rlog_t0, *rlog_val;
    uint32_t *rlog_key;
    double *cterm;          // [B][cpad] scratch: per-channel term of calculate_total_r_spatial while a launch keeps the per-step
                            // totals incrementally (not part of the state: rebuilt at the start of every launch that needs it)
    const uint8_t *mod_t;   // [num_rows*K][cpad] modulation level per channel
    const uint32_t *mod_k;  // [num_rows][cpad][2] the same, the levels of one channel on all K paths together (bytes 0..K-1)
    const double *gsnr_t;   // [num_rows*K][cpad]
    // per-call IO
    const int32_t *act_path;      // external actions: [B] path (-2 = blocked)
    const int16_t *act_channels;  // [B][ORLG_PHY_MAX_CH], -1 terminated; channel | used << 9 (used 0 = the full capacity)
    void *outs[ORLG_PHY_NUM_OUTS];
    int32_t *err_flag;            // the handle's sticky error word (mapped host memory): a queue / list overflow happened
    // per-wave LDS layout
    int32_t l_occ, l_nbt, l_nbi, l_scratch, l_wsc, l_wave_bytes, l_shared_bytes, l_outs;
    int32_t l_mtstage;      // the workgroup's MT19937 staging buffer (2496 B, then its lock word), after the tables
    // per-environment traffic (orlg_phy_create_traffic): [B] pairs that take the place of arrival_lambda / holding_lambda above,
    // nullptr = every environment has the scalars.  Read where a refill or nb_rebuild needs it (orlg_env_rates), never kept
    const OrlgRates *rates;
    // request trace (orlg_phy_create_trace), as OrlgParams::tr_*: [B][tr_len] each, nullptr = generated traffic; the cursor of an
    // environment lives in OrlgPhyScalars::mt_idx, the ring's first array holds absolute arrival times
    const double *tr_arrival, *tr_holding;
    const uint32_t *tr_req;
    int32_t tr_len, pad_tr;
};

struct PhyWaveScalars {  // LDS
    int64_t c[8];
    int64_t total_path_index, total_mod, channels_accepted, physical_accepted, episodes_done;
    double total_path_length, total_gsnr, req_arrival, req_holding;
    int32_t q_overflow, counted_moves, counted_moves_groom, counted_defrag_cycles;
};

// the links of one path record as a bit mask over the link index (networks of at most 32 links: US14, NSFNET, JPN12):
// the RSS metric works on one channel's column along the link axis as a 32-bit vector
struct OrlgPathMasks { uint32_t path; };

struct PhyTab {
    const OrlgPathMasks *masks;
    const int32_t *pair_base;
    const OrlgPathRec *recs;
    const int32_t *bit_rates;
    const double *br_cum, *src_cum, *dst_cum;
    const int32_t *pair_row;
    const int32_t *adj_off;    // [num_paths+1]
    const uint16_t *adj;       // link | weight << 8
    const double *sqrt_tab;    // sqrt(k), k = 0..E*E
    const double *path_len;    // [num_paths]
    const uint16_t *path_pair; // [num_paths] a * N + b of the pair (a < b) the record belongs to
    const uint64_t *outs;
    const uint64_t *lnib;      // [E] 1 << 4 a | 1 << 4 b for a link a - b (only with OrlgPhyParams::use_nv)
};

DEV PhyTab make_phy_tab(unsigned char *smem, const OrlgPhyParams &p) {
    PhyTab tb;
    tb.pair_base = reinterpret_cast<const int32_t *>(smem + p.t_pair);
    tb.recs = reinterpret_cast<const OrlgPathRec *>(smem + p.t_recs);
    tb.bit_rates = reinterpret_cast<const int32_t *>(smem + p.t_bitrates);
    tb.br_cum = reinterpret_cast<const double *>(smem + p.t_brcum);
    tb.src_cum = reinterpret_cast<const double *>(smem + p.t_srccum);
    tb.dst_cum = reinterpret_cast<const double *>(smem + p.t_dstcum);
    tb.pair_row = reinterpret_cast<const int32_t *>(smem + p.t_pairrow);
    tb.adj_off = reinterpret_cast<const int32_t *>(smem + p.t_adjoff);
    tb.adj = reinterpret_cast<const uint16_t *>(smem + p.t_adj);
    tb.sqrt_tab = reinterpret_cast<const double *>(smem + p.t_sqrt);
    tb.path_len = reinterpret_cast<const double *>(smem + p.t_plen);
    tb.path_pair = reinterpret_cast<const uint16_t *>(smem + p.t_pathpair);
    tb.masks = reinterpret_cast<const OrlgPathMasks *>(smem + p.t_masks);
    tb.outs = reinterpret_cast<const uint64_t *>(smem + p.l_outs);
    tb.lnib = reinterpret_cast<const uint64_t *>(smem + p.t_lnib);
    return tb;
}
