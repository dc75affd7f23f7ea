// orlg_inst_gnadmit.hip -- instantiations of orlg_gn_admission_masks_kernel and orlg_gn_admission_windows_kernel
// (orlg_gn_admission_kernels.hip: the masks and rule windows that know both halves of the GN-model admission check) for ONE word
// count, -DORLG_INST_W=<W>: one object per W next to the orlg_inst_wave, orlg_inst_gnrules and orlg_inst_gnprotect objects, which
// hold what they held.
#include "orlg_host.h"
#include "orlg_gn_admission_kernels.hip"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

orlg_gn_admission_masks_kernel_t ORLG_CAT(orlg_gn_admission_masks_kernel_W, ORLG_INST_W)() { return orlg_gn_admission_masks_kernel<ORLG_INST_W>; }
orlg_gn_admission_windows_kernel_t ORLG_CAT(orlg_gn_admission_windows_kernel_W, ORLG_INST_W)() { return orlg_gn_admission_windows_kernel<ORLG_INST_W>; }
