// orlg_inst_gnslots.hip -- the instantiation of orlg_gn_slots_kernel (orlg_gn_slots_kernels.hip: the GN-model admission check over
// every start slot of every candidate path) for one word count (orlg_inst.h).
#include "orlg_host.h"
#include "orlg_gn_slots_kernels.hip"
#include "orlg_inst.h"

ORLG_INST_QUERY(orlg_gn_slots_kernel_t, orlg_gn_slots_kernel_W, orlg_gn_slots_kernel)
