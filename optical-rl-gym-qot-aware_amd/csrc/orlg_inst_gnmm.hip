// orlg_inst_gnmm.hip -- instantiations of the gated wave-per-environment step kernel under a max-margin policy (orlg_kernels.hip,
// orlg_rmsa_mm_kernel = rmsa_body<.., GN, .., MM>: what orlg_step_max_margin launches) for ONE word count, -DORLG_INST_W=<W>: one object
// per W next to the orlg_inst_wave, orlg_inst_gnrules, orlg_inst_gnprotect, orlg_inst_gnadmit and orlg_inst_gnslots objects, which hold
// what they held.  Which ones: orlg_variants.h, ORLG_WAVE_GN_MM_KEYS.
#include "orlg_host.h"
#include "orlg_kernels.hip"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

orlg_rmsa_mm_kernel_t ORLG_CAT(orlg_gnmm_kernel_W, ORLG_INST_W)(OrlgMmKey key) {
#define X(...) if (key == OrlgMmKey{__VA_ARGS__}) return orlg_rmsa_mm_kernel<ORLG_INST_W, __VA_ARGS__>;
    ORLG_WAVE_GN_MM_KEYS(X)
#undef X
    return nullptr;
}
