// orlg_inst_gnam.hip -- instantiations of the gated wave-per-environment step kernel of a handle whose gate chooses the modulation from
// the GSNR (orlg_kernels.hip, orlg_rmsa_am_kernel = rmsa_body<.., GN, .., AM>: what every step of such a handle launches) and of
// orlg_gn_modulation_kernel (orlg_gn_modulation_kernels.hip) for one word count (orlg_inst.h).  Which ones:
// orlg_variants.h, ORLG_WAVE_GN_AM_KEYS.
#include "orlg_host.h"
#include "orlg_kernels.hip"
#include "orlg_gn_modulation_kernels.hip"
#include "orlg_inst.h"

ORLG_INST_LOOKUP(orlg_rmsa_am_kernel_t, orlg_gnam_kernel_W, OrlgAmKey, ORLG_WAVE_GN_AM_KEYS, ORLG_INST_AM)
ORLG_INST_QUERY(orlg_gn_modulation_kernel_t, orlg_gn_modulation_kernel_W, orlg_gn_modulation_kernel)
