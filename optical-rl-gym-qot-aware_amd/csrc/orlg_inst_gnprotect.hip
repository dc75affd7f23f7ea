// orlg_inst_gnprotect.hip -- instantiations of the wave-per-environment step kernel with the GN-model admission check AND the check
// of the running lightpaths (orlg_kernels.hip, rmsa_body<.., GN, .., PROTECT>: what a handle with orlg_set_gn_protect launches) for
// ONE word count, -DORLG_INST_W=<W>: one object per W next to the orlg_inst_wave and orlg_inst_gnrules objects, which hold what they
// held.  Which ones: orlg_variants.h, ORLG_WAVE_GN_PROTECT_KEYS and ORLG_WAVE_GN_PROTECT_CAUSE_KEYS.
#include "orlg_host.h"
#include "orlg_kernels.hip"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

orlg_rmsa_kernel_t ORLG_CAT(orlg_gnprotect_kernel_W, ORLG_INST_W)(OrlgWaveKey key) {
#define X(name, ...) if (key == OrlgWaveKey{ORLG_WAVE_KERNEL(name), __VA_ARGS__}) return name<ORLG_INST_W, __VA_ARGS__>;
    ORLG_WAVE_GN_PROTECT_KEYS(X)
    ORLG_WAVE_GN_PROTECT_CAUSE_KEYS(X)
#undef X
    return nullptr;
}
