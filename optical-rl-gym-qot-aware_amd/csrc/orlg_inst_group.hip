// orlg_inst_group.hip -- instantiations of the four-environments-per-wave step kernel (orlg_group_kernels.hip) for ONE word
// count, -DORLG_INST_W=<W> (see orlg_inst_wave.hip).  Which ones: orlg_variants.h.
#include "orlg_host.h"
#include "orlg_group_kernels.hip"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

orlg_rmsa_kernel_t ORLG_CAT(orlg_group_kernel_W, ORLG_INST_W)(OrlgGroupKey key) {
#define X(...) if (key == OrlgGroupKey{__VA_ARGS__}) return orlg_rmsa_group_kernel<ORLG_INST_W, __VA_ARGS__>;
    ORLG_GROUP_KEYS(X)
    ORLG_GROUP_CAUSE_KEYS(X)
    ORLG_GROUP_ASSIGN_KEYS(X)
    ORLG_GROUP_CUT_KEYS(X)
    ORLG_GROUP_USAGE_KEYS(X)
#undef X
    return nullptr;
}
