// orlg_inst_gnprotect.hip -- instantiations of the wave-per-environment step kernel with the GN-model admission check AND the check
// of the running lightpaths (orlg_kernels.hip, rmsa_body<.., GN, .., PROTECT>: what a handle with orlg_set_gn_protect launches) for
// one word count (orlg_inst.h).  Which ones: orlg_variants.h, ORLG_GNPROTECT_UNIT_KEYS.
#include "orlg_host.h"
#include "orlg_kernels.hip"
#include "orlg_inst.h"

ORLG_INST_LOOKUP(orlg_rmsa_kernel_t, orlg_gnprotect_kernel_W, OrlgWaveKey, ORLG_GNPROTECT_UNIT_KEYS, ORLG_INST_WAVE)
