// orlg_inst_phy.hip -- instantiations of the QoT-aware step kernel (orlg_phy_kernels.hip) for one word count
// (orlg_inst.h), and one half of the keys of orlg_variants.h: -DORLG_INST_TRACE=1 makes the TRACE instantiations
// (handles that replay a request trace), objects of their own so that they compile next to the others and not after them.
#include "orlg_host.h"
#include "orlg_phy_kernels.hip"
#include "orlg_inst.h"

#if defined(ORLG_INST_TRACE) && ORLG_INST_TRACE
orlg_phy_kernel_t ORLG_CAT(orlg_phy_trace_kernel_W, ORLG_INST_W)(OrlgPhyKey key) {
    constexpr bool TRACE = true;
#else
orlg_phy_kernel_t ORLG_CAT(orlg_phy_kernel_W, ORLG_INST_W)(OrlgPhyKey key) {
    constexpr bool TRACE = false;
#endif
    ORLG_PHY_KEYS_OF(ORLG_INST_PHY, TRACE)
    return nullptr;
}
