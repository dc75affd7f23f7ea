// orlg_inst_phy.hip -- instantiations of the QoT-aware step kernel (orlg_phy_kernels.hip) for ONE word count, -DORLG_INST_W=<W>
// (see orlg_inst_wave.hip), and one half of the keys of orlg_variants.h: -DORLG_INST_TRACE=1 makes the TRACE instantiations
// (handles that replay a request trace), objects of their own so that they compile next to the others and not after them.
#include "orlg_host.h"
#include "orlg_phy_kernels.hip"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

#if defined(ORLG_INST_TRACE) && ORLG_INST_TRACE
orlg_phy_kernel_t ORLG_CAT(orlg_phy_trace_kernel_W, ORLG_INST_W)(OrlgPhyKey key) {
    constexpr bool TRACE = true;
#else
orlg_phy_kernel_t ORLG_CAT(orlg_phy_kernel_W, ORLG_INST_W)(OrlgPhyKey key) {
    constexpr bool TRACE = false;
#endif
#define X(...) if (key == OrlgPhyKey{__VA_ARGS__}) return orlg_phy_kernel<ORLG_INST_W, __VA_ARGS__>;
    ORLG_PHY_KEYS_OF(X, TRACE)
#undef X
    return nullptr;
}
