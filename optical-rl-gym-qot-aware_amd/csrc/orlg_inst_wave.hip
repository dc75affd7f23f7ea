// orlg_inst_wave.hip -- instantiations of the wave-per-environment kernels (orlg_kernels.hip, and the query and mask kernels of
// orlg_query_kernels.hip, orlg_mask_kernels.hip and orlg_gn_mask_kernels.hip, in the order the file always met them; orlg_fit_levels_kernel
// of orlg_block_cause.h, orlg_min_cuts_kernel of orlg_cut.h and orlg_usage_kernel of orlg_usage.h last) for ONE word count,
// -DORLG_INST_W=<W>: one object per W, so that the library builds in parallel (build.py).  Which ones: orlg_variants.h.
#include "orlg_host.h"
#include "orlg_kernels.hip"
#include "orlg_query_kernels.hip"
#include "orlg_mask_kernels.hip"
#include "orlg_gn_mask_kernels.hip"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

orlg_rmsa_kernel_t ORLG_CAT(orlg_wave_kernel_W, ORLG_INST_W)(OrlgWaveKey key) {
#define X(name, ...) if (key == OrlgWaveKey{ORLG_WAVE_KERNEL(name), __VA_ARGS__}) return name<ORLG_INST_W, __VA_ARGS__>;
    ORLG_WAVE_KEYS(X)
    ORLG_WAVE_GN_KEYS(X)
    ORLG_WAVE_CAUSE_KEYS(X)
    ORLG_WAVE_ASSIGN_KEYS(X)
    ORLG_WAVE_CUT_KEYS(X)
    ORLG_WAVE_USAGE_KEYS(X)
#undef X
    return nullptr;
}
orlg_masks_kernel_t ORLG_CAT(orlg_masks_kernel_W, ORLG_INST_W)() { return orlg_path_masks_kernel<ORLG_INST_W>; }
orlg_obs_kernel_t ORLG_CAT(orlg_obs_kernel_W, ORLG_INST_W)() { return orlg_deeprmsa_obs_kernel<ORLG_INST_W>; }
orlg_action_masks_kernel_t ORLG_CAT(orlg_action_masks_kernel_W, ORLG_INST_W)() { return orlg_action_masks_kernel<ORLG_INST_W>; }
orlg_gn_action_masks_kernel_t ORLG_CAT(orlg_gn_action_masks_kernel_W, ORLG_INST_W)() { return orlg_gn_action_masks_kernel<ORLG_INST_W>; }
orlg_fit_levels_kernel_t ORLG_CAT(orlg_fit_levels_kernel_W, ORLG_INST_W)() { return orlg_fit_levels_kernel<ORLG_INST_W>; }
orlg_min_cuts_kernel_t ORLG_CAT(orlg_min_cuts_kernel_W, ORLG_INST_W)() { return orlg_min_cuts_kernel<ORLG_INST_W>; }
orlg_usage_kernel_t ORLG_CAT(orlg_usage_kernel_W, ORLG_INST_W)() { return orlg_usage_kernel<ORLG_INST_W>; }
