// orlg_inst_group.hip -- instantiations of the four-environments-per-wave step kernel (orlg_group_kernels.hip) for one word count
// (orlg_inst.h).  Which ones: orlg_variants.h, ORLG_GROUP_UNIT_KEYS.
#include "orlg_host.h"
#include "orlg_group_kernels.hip"
#include "orlg_inst.h"

ORLG_INST_LOOKUP(orlg_rmsa_kernel_t, orlg_group_kernel_W, OrlgGroupKey, ORLG_GROUP_UNIT_KEYS, ORLG_INST_GROUP)
