// orlg_inst_phy_trace.hip -- the TRACE instantiations of the QoT-aware step kernel (handles that replay a request trace,
// OrlgPhyParams::tr_*) for ONE word count, -DORLG_INST_W=<W>: objects of their own, so that they compile next to
// orlg_inst_phy.hip and not after it.  Variants as there.
#include "orlg_host.h"
#include "orlg_phy_kernels.hip"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

#define ORLG_PHY_POL_CASES(base, POL)                                                     \
    case base: return orlg_phy_kernel<ORLG_INST_W, false, false, POL, false, true>;       \
    case base + 1: return orlg_phy_kernel<ORLG_INST_W, true, false, POL, false, true>;    \
    case base + 2: return orlg_phy_kernel<ORLG_INST_W, true, true, POL, false, true>;     \
    case base + 3: return orlg_phy_kernel<ORLG_INST_W, false, true, POL, false, true>;
#define ORLG_PHY_CONT_CASES(base, POL)                                                    \
    case base: return orlg_phy_kernel<ORLG_INST_W, false, false, POL, true, true>;        \
    case base + 1: return orlg_phy_kernel<ORLG_INST_W, false, true, POL, true, true>;
orlg_phy_kernel_t ORLG_CAT(orlg_phy_trace_kernel_W, ORLG_INST_W)(int variant) {
    switch (variant) {
        ORLG_PHY_POL_CASES(0, ORLG_PHY_POLICY_EXTERNAL)
        ORLG_PHY_POL_CASES(4, ORLG_PHY_POLICY_BMFA_CUT)
#ifndef ORLG_PHY_FEW_POLICIES
        ORLG_PHY_POL_CASES(8, ORLG_PHY_POLICY_BMFA_RSS_METRIC)
        ORLG_PHY_POL_CASES(12, ORLG_PHY_POLICY_SAPFF)
        ORLG_PHY_POL_CASES(16, ORLG_PHY_POLICY_BMFF)
        ORLG_PHY_POL_CASES(20, ORLG_PHY_POLICY_SAPBM)
        ORLG_PHY_POL_CASES(24, ORLG_PHY_POLICY_FAFF)
        ORLG_PHY_POL_CASES(28, ORLG_PHY_POLICY_FAFF_RSS)
        ORLG_PHY_CONT_CASES(32, ORLG_PHY_POLICY_EXTERNAL)
        ORLG_PHY_CONT_CASES(34, ORLG_PHY_POLICY_BMFA_CUT)
        ORLG_PHY_CONT_CASES(36, ORLG_PHY_POLICY_BMFA_RSS_METRIC)
        ORLG_PHY_CONT_CASES(38, ORLG_PHY_POLICY_SAPFF)
        ORLG_PHY_CONT_CASES(40, ORLG_PHY_POLICY_BMFF)
        ORLG_PHY_CONT_CASES(42, ORLG_PHY_POLICY_SAPBM)
        ORLG_PHY_CONT_CASES(44, ORLG_PHY_POLICY_FAFF)
        ORLG_PHY_CONT_CASES(46, ORLG_PHY_POLICY_FAFF_RSS)
#endif
        default: return nullptr;
    }
}
