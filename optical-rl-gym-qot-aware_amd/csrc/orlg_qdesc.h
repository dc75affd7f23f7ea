// orlg_qdesc.h -- the descriptor of a running service in the release ring (OrlgParams::qdesc) on a handle whose gate chooses the
// modulation from the GSNR (orlg_set_gn_modulation), decoded ONCE: every reader of a descriptor that may carry a level
// goes through here -- the release and the check of the AM step kernel (orlg_kernels.hip, orlg_rmsa_gn_am.h), the modulation query
// (orlg_gn_modulation_kernels.hip), the audit and the list of the running services (orlg_gn_audit_kernels.hip).
//
// Every handle:       path record, 14 bits | first slot << 14, 10 bits | bit-rate index << 24, 8 bits
// An adaptive handle: path record, 11 bits | level << 11, 3 bits | first slot << 14 | bit-rate index << 24
// The level is the spectral efficiency the service runs at, 1 .. M; 0 = the path's own (what every policy that does not choose a level
// stores), so a state without adaptive services reads the same either way.  An adaptive handle has fewer than 2048 path records
// (refused otherwise), and a handle that is not adaptive never sees a level: orlg_load_state refuses such a snapshot.
// Plain C++: the host includes it too.
#pragma once
#include <stdint.h>

#define ORLG_QDESC_AM_PATHS 2048   // path records an adaptive handle may have (exclusive)
#define ORLG_QDESC_MAX_LEVEL 6     // the modulation factors of the GN model end at spectral efficiency 6 (orlg_rmsa_gn.h)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ORLG_QD __host__ __device__ inline __attribute__((always_inline))
#else
#define ORLG_QD static inline
#endif

// adaptive: the handle's mode (OrlgParams::gn_adaptive != 0)
ORLG_QD int orlg_qdesc_gid(uint32_t d, bool adaptive) { return (int)(d & (adaptive ? 0x7ffu : 0x3fffu)); }
ORLG_QD int orlg_qdesc_level(uint32_t d, bool adaptive) { return adaptive ? (int)((d >> 11) & 7u) : 0; }
ORLG_QD int orlg_qdesc_slot(uint32_t d) { return (int)((d >> 14) & 0x3ffu); }
ORLG_QD int orlg_qdesc_rate(uint32_t d) { return (int)(d >> 24); }
// the spectral efficiency a service runs at: its stored level, or its path's own
ORLG_QD int orlg_qdesc_se(int level, int path_se) { return level ? level : path_se; }
ORLG_QD uint32_t orlg_qdesc_make(int gid, int level, int slot, int rate) {
    return (uint32_t)gid | ((uint32_t)level << 11) | ((uint32_t)slot << 14) | ((uint32_t)rate << 24);
}
