// orlg_inst_gnadmit.hip -- instantiations of orlg_gn_admission_masks_kernel and orlg_gn_admission_windows_kernel
// (orlg_gn_admission_kernels.hip: the masks and rule windows that know both halves of the GN-model admission check) for one word
// count (orlg_inst.h).
#include "orlg_host.h"
#include "orlg_gn_admission_kernels.hip"
#include "orlg_inst.h"

ORLG_INST_QUERY(orlg_gn_admission_masks_kernel_t, orlg_gn_admission_masks_kernel_W, orlg_gn_admission_masks_kernel)
ORLG_INST_QUERY(orlg_gn_admission_windows_kernel_t, orlg_gn_admission_windows_kernel_W, orlg_gn_admission_windows_kernel)
