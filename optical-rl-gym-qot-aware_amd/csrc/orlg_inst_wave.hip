// orlg_inst_wave.hip -- instantiations of the wave-per-environment kernels (orlg_kernels.hip, and the query and mask kernels of
// orlg_query_kernels.hip, orlg_mask_kernels.hip and orlg_gn_mask_kernels.hip, in the order the file always met them; orlg_fit_levels_kernel
// of orlg_block_cause.h, orlg_min_cuts_kernel of orlg_cut.h and orlg_usage_kernel of orlg_usage.h last) for one word count
// (orlg_inst.h).  Which ones: orlg_variants.h, ORLG_WAVE_UNIT_KEYS.
#include "orlg_host.h"
#include "orlg_kernels.hip"
#include "orlg_query_kernels.hip"
#include "orlg_mask_kernels.hip"
#include "orlg_gn_mask_kernels.hip"
#include "orlg_inst.h"

ORLG_INST_LOOKUP(orlg_rmsa_kernel_t, orlg_wave_kernel_W, OrlgWaveKey, ORLG_WAVE_UNIT_KEYS, ORLG_INST_WAVE)
ORLG_INST_QUERY(orlg_masks_kernel_t, orlg_masks_kernel_W, orlg_path_masks_kernel)
ORLG_INST_QUERY(orlg_obs_kernel_t, orlg_obs_kernel_W, orlg_deeprmsa_obs_kernel)
ORLG_INST_QUERY(orlg_action_masks_kernel_t, orlg_action_masks_kernel_W, orlg_action_masks_kernel)
ORLG_INST_QUERY(orlg_gn_action_masks_kernel_t, orlg_gn_action_masks_kernel_W, orlg_gn_action_masks_kernel)
ORLG_INST_QUERY(orlg_fit_levels_kernel_t, orlg_fit_levels_kernel_W, orlg_fit_levels_kernel)
ORLG_INST_QUERY(orlg_min_cuts_kernel_t, orlg_min_cuts_kernel_W, orlg_min_cuts_kernel)
ORLG_INST_QUERY(orlg_usage_kernel_t, orlg_usage_kernel_W, orlg_usage_kernel)
