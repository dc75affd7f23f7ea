// orlg_inst_gnam.hip -- instantiations of the gated wave-per-environment step kernel of a handle whose gate chooses the modulation from
// the GSNR (orlg_kernels.hip, orlg_rmsa_am_kernel = rmsa_body<.., GN, .., AM>: what every step of such a handle launches) and of
// orlg_gn_modulation_kernel (orlg_gn_modulation_kernels.hip) for ONE word count, -DORLG_INST_W=<W>: one object per W next to the
// orlg_inst_wave, orlg_inst_gnrules, orlg_inst_gnprotect, orlg_inst_gnadmit, orlg_inst_gnslots and orlg_inst_gnmm objects, which hold
// what they held.  Which ones: orlg_variants.h, ORLG_WAVE_GN_AM_KEYS.
#include "orlg_host.h"
#include "orlg_kernels.hip"
#include "orlg_gn_modulation_kernels.hip"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

orlg_rmsa_am_kernel_t ORLG_CAT(orlg_gnam_kernel_W, ORLG_INST_W)(OrlgAmKey key) {
#define X(...) if (key == OrlgAmKey{__VA_ARGS__}) return orlg_rmsa_am_kernel<ORLG_INST_W, __VA_ARGS__>;
    ORLG_WAVE_GN_AM_KEYS(X)
#undef X
    return nullptr;
}
orlg_gn_modulation_kernel_t ORLG_CAT(orlg_gn_modulation_kernel_W, ORLG_INST_W)() { return orlg_gn_modulation_kernel<ORLG_INST_W>; }
