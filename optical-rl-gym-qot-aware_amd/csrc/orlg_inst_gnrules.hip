// orlg_inst_gnrules.hip -- instantiations of the wave-per-environment step kernel with the GN-model admission check AND an assignment
// rule (orlg_kernels.hip, rmsa_body<.., GN, .., ASSIGN[, CUT]>: what orlg_step_rule_gn launches) and of orlg_gn_path_windows_kernel
// (orlg_gn_rule_kernels.hip) for one word count (orlg_inst.h).  Which ones: orlg_variants.h, ORLG_GNRULES_UNIT_KEYS.
#include "orlg_host.h"
#include "orlg_kernels.hip"
#include "orlg_gn_rule_kernels.hip"
#include "orlg_inst.h"

ORLG_INST_LOOKUP(orlg_rmsa_kernel_t, orlg_gnrules_kernel_W, OrlgWaveKey, ORLG_GNRULES_UNIT_KEYS, ORLG_INST_WAVE)
ORLG_INST_QUERY(orlg_gn_path_windows_kernel_t, orlg_gn_path_windows_kernel_W, orlg_gn_path_windows_kernel)
