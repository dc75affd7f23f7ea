// orlg_rmsa_host.h -- what the three translation units of the RMSA C API (include/orlg.h) share: the handle, the slots of its extra
// buffers and the two functions that cross units.
//   orlg_api.hip        the helper kernels, create, reset, reseed, the getters and reductions, checkpoint / resume, the debug exports
//   orlg_api_step.hip   launch_rmsa and the group kernel's launch, rmsa_step and the orlg_step* entries, orlg_launch_info, the gate:
//                       gn_gate_table, orlg_set_gn_gate, orlg_set_gn_protect, orlg_set_gn_modulation with orlg_step_modulation
//   orlg_api_query.hip  what reads the state with a kernel of orlg_query_kernels.hip, orlg_mask_kernels.hip or the orlg_gn_*_kernels:
//                       path masks, the DeepRMSA observation, action masks, fit levels, cuts, usage, the GN masks and windows, the
//                       running services and their audit -- with the output slots of a query and the queries' one launch
// No unit needs more of another than this header; with the QoT-aware API they share the handle core of orlg_host.h.
#pragma once
#include "orlg_host.h"
#include "orlg_group_plan.h"
#include "orlg_wave_plan.h"

// ---------------------------------------------------------------------------------------- handle
struct orlg_env : OrlgHandle {
    OrlgParams p = {};
    int resident_blocks = 0;   // workgroups of the step kernel the device keeps resident (grid size of the work queue)
    // four-environments-per-wave step kernel: group_mode = ORLG_KERNEL_* (AUTO falls back to WAVE when the shape does not fit the
    // kernel's LDS budget); the LDS layout of each kind of instantiation (orlg_group_plan.h) and its resident workgroups
    int group_mode = 0;
    OrlgGroupLayout group[3] = {};                          // by OrlgGroupKind
    int group_usage_resident[ORLG_GROUP_WAVES + 1] = {};    // ... of the USAGE instantiations, which take more LDS (launch_rmsa_group)
    int group_resident[3][ORLG_GROUP_WAVES + 1] = {};       // ... by waves per workgroup (0 = not asked yet)
    uint4 *llog = nullptr;          // DEFER: the log of link updates [B][E][ORLG_LLOG_CAP] (allocated with the first such launch)
    uint32_t *progress = nullptr;   // chunked tickets: chunks completed per quad in the current launch (allocated with the first such launch)
    int allow_rejection = 0;   // the action spaces carry the explicit rejection (orlg_set_allow_rejection): one more mask column
    int min_slots = 1;   // the smallest entry of the slots table (0 where a bit rate is negative: such a handle keeps the full body)
    std::vector<uint8_t> path_se;   // spectral efficiency of every path record (orlg_set_gn_gate checks the thresholds against it)
    double *gn_table = nullptr;     // the gate's table on the device (allocated with the first gate; OrlgParams::gn = it or nullptr)
    bool gn_protect = false;        // the gate also protects the running lightpaths (orlg_set_gn_protect; configuration, not state)
    double *audit_table = nullptr;  // the table of a gate given with orlg_gn_audit (allocated with the first such call; never OrlgParams::gn)
    int mm_resident[3][2] = {};     // workgroups of orlg_rmsa_mm_kernel the device keeps resident, by statistics level and CAUSE (0 = not asked yet)
    int gn_num_thresholds = 0;      // num_thresholds of the gate in force: the levels a gate that chooses the modulation has (orlg_set_gn_modulation)
    int am_resident[3] = {};       // ... of orlg_rmsa_am_kernel, by statistics level (the gate's mode itself is OrlgParams::gn_adaptive)
};
enum { X_ACTIONS, X_GSNR, X_CAUSE, X_CAUSE_COUNTS, X_MARGIN, X_WINDOW_MARGIN, X_SE };   // OrlgHandle::extra: external actions from / the gn_gsnr_db, block_cause, cause_counts, gn_neighbour_margin_db and gn_window_margin_db outputs for host memory
static_assert(X_SE < ORLG_EXTRA_SLOTS, "OrlgHandle::extra");   // (X_SE: the gn_se output of orlg_step_modulation)

#define SYNC_CHECK(e) do { int rc_ = orlg_handle_sync_check(e); if (rc_) return rc_; } while (0)

// ---------------------------------------------------------------------------------------- across the units (orlg_api_step.hip)
// one launch of the step kernel that serves p (p.mode: a step, the initial reset or an episode reset)
int launch_rmsa(orlg_env *e, const OrlgParams &p);
// the rules of a gate and its table (ORLG_GN_*, orlg_device.h) for this handle's topology: what orlg_set_gn_gate installs and what
// orlg_gn_audit builds for a gate given with the call
int gn_gate_table(const orlg_env *e, const orlg_rmsa_gn_gate *g, std::vector<double> &tab);
// 1 where a descriptor of `qdesc` (B * Q words, host or device memory: a state blob's part or the handle's own array) names no path
// record of the handle -- what the level of an adaptive handle's service looks like to a handle that is not (orlg_qdesc.h); 0 where
// none does; a negative error code
int rmsa_state_has_levels(orlg_env *e, const void *qdesc);
