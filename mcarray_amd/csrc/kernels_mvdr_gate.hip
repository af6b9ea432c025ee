// kernels_mvdr_gate.hip -- the MVDR solve with a per-frame covariance update weight (gfx950; include/mcarray_hip.h,
// mca_hip_mvdr_sources_frames_weighted_dev): the instantiations of mvdr_gate.h without the noise plane.  A
// translation unit and an argument struct of their own, so that the unweighted kernels of kernels_mvdr.hip and
// kernels_mvdr_nulls.hip keep their code objects (kernels_mvdr_nulls.hip on why).
#include "mvdr_gate.h"

namespace mca {

#define MCA_MVDR_GATE_PLAIN_INST(Q, S, S1F, S1P, RF, RP)                                                  \
    template __global__ void k_mvdr_gated_t<Q, true, S, S1F, true, false, RF, false>(MvdrGateArgs);          \
    template __global__ void k_mvdr_gated_t<Q, false, S, S1P, true, false, RP, false>(MvdrGateArgs);
MCA_MVDR_GATE_PLAIN_TABLE(MCA_MVDR_GATE_PLAIN_INST)
#undef MCA_MVDR_GATE_PLAIN_INST
#define MCA_MVDR_GATE_NULLS_INST(Q, S, S1, PF, R) template __global__ void k_mvdr_gated_t<Q, false, S, S1, PF, true, R, false>(MvdrGateArgs);
MCA_MVDR_GATE_NULLS_TABLE(MCA_MVDR_GATE_NULLS_INST)
#undef MCA_MVDR_GATE_NULLS_INST

}  // namespace mca
