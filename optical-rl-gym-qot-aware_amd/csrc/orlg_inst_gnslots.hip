// orlg_inst_gnslots.hip -- the instantiation of orlg_gn_slots_kernel (orlg_gn_slots_kernels.hip: the GN-model admission check over
// every start slot of every candidate path) for ONE word count, -DORLG_INST_W=<W>: one object per W next to the orlg_inst_wave,
// orlg_inst_gnrules, orlg_inst_gnprotect and orlg_inst_gnadmit objects, which hold what they held.
#include "orlg_host.h"
#include "orlg_gn_slots_kernels.hip"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

orlg_gn_slots_kernel_t ORLG_CAT(orlg_gn_slots_kernel_W, ORLG_INST_W)() { return orlg_gn_slots_kernel<ORLG_INST_W>; }
