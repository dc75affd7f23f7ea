// orlg_inst_gnmm.hip -- instantiations of the gated wave-per-environment step kernel under a max-margin policy (orlg_kernels.hip,
// orlg_rmsa_mm_kernel = rmsa_body<.., GN, .., MM>: what orlg_step_max_margin launches) for one word count (orlg_inst.h).
// Which ones: orlg_variants.h, ORLG_WAVE_GN_MM_KEYS.
#include "orlg_host.h"
#include "orlg_kernels.hip"
#include "orlg_inst.h"

ORLG_INST_LOOKUP(orlg_rmsa_mm_kernel_t, orlg_gnmm_kernel_W, OrlgMmKey, ORLG_WAVE_GN_MM_KEYS, ORLG_INST_MM)
