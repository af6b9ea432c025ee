// kernels_mvdr_mask.hip -- the MVDR solve with a covariance update weight per frame and bin (gfx950; include/mcarray_hip.h,
// mca_hip_mvdr_sources_frames_masked_dev): k_mvdr_masked_t, the body of mvdr_gate.h with the weight read at
// update_mask[(a F + t) K + k], in the instantiations of kernels_mvdr_gate.hip (no noise plane).  A translation unit and kernel
// names of their own, so that the per-frame kernels keep their code objects.
#include "mvdr_gate.h"

namespace mca {

#define MCA_MVDR_MASK_PLAIN_INST(Q, S, S1F, S1P, RF, RP)                                                   \
    template __global__ void k_mvdr_masked_t<Q, true, S, S1F, MCA_MVDR_MASK_PF(Q, S), false, false, false>(MvdrGateArgs);          \
    template __global__ void k_mvdr_masked_t<Q, false, S, S1P, MCA_MVDR_MASK_PF(Q, S), false, false, false>(MvdrGateArgs);
MCA_MVDR_GATE_PLAIN_TABLE(MCA_MVDR_MASK_PLAIN_INST)
#undef MCA_MVDR_MASK_PLAIN_INST
#define MCA_MVDR_MASK_NULLS_INST(Q, S, S1, PF, R) template __global__ void k_mvdr_masked_t<Q, false, S, S1, PF && MCA_MVDR_MASK_PF(Q, S), true, false, false>(MvdrGateArgs);
MCA_MVDR_GATE_NULLS_TABLE(MCA_MVDR_MASK_NULLS_INST)
#undef MCA_MVDR_MASK_NULLS_INST

}  // namespace mca
