// orlg_inst_gnrules.hip -- instantiations of the wave-per-environment step kernel with the GN-model admission check AND an assignment
// rule (orlg_kernels.hip, rmsa_body<.., GN, .., ASSIGN[, CUT]>: what orlg_step_rule_gn launches) and of orlg_gn_path_windows_kernel
// (orlg_gn_rule_kernels.hip) for ONE word count, -DORLG_INST_W=<W>: one object per W next to the orlg_inst_wave objects, which
// hold what they held.  Which ones: orlg_variants.h, ORLG_WAVE_GN_ASSIGN_KEYS and ORLG_WAVE_GN_CUT_KEYS.
#include "orlg_host.h"
#include "orlg_kernels.hip"
#include "orlg_gn_rule_kernels.hip"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

orlg_rmsa_kernel_t ORLG_CAT(orlg_gnrules_kernel_W, ORLG_INST_W)(OrlgWaveKey key) {
#define X(name, ...) if (key == OrlgWaveKey{ORLG_WAVE_KERNEL(name), __VA_ARGS__}) return name<ORLG_INST_W, __VA_ARGS__>;
    ORLG_WAVE_GN_ASSIGN_KEYS(X)
    ORLG_WAVE_GN_CUT_KEYS(X)
#undef X
    return nullptr;
}
orlg_gn_path_windows_kernel_t ORLG_CAT(orlg_gn_path_windows_kernel_W, ORLG_INST_W)() { return orlg_gn_path_windows_kernel<ORLG_INST_W>; }
