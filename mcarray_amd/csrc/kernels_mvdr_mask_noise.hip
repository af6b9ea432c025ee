// kernels_mvdr_mask_noise.hip -- the masked MVDR solve that also emits the residual noise power of every output (gfx950;
// include/mcarray_hip.h, mca_hip_mvdr_sources_frames_masked_dev with the post-filter enabled): the NOISE = true
// instantiations of k_mvdr_masked_t, those of kernels_mvdr_gate_noise.hip.  A translation unit of their own like theirs.
#include "mvdr_gate.h"

namespace mca {

#define MCA_MVDR_MASK_NOISE_PLAIN_INST(Q, S, S1F, S1P, PFP, RF, RP)                                             \
    template __global__ void k_mvdr_masked_t<Q, true, S, S1F, MCA_MVDR_MASK_PF(Q, S), false, false, true>(MvdrGateNoiseArgs);          \
    template __global__ void k_mvdr_masked_t<Q, false, S, S1P, PFP && MCA_MVDR_MASK_PF(Q, S), false, false, true>(MvdrGateNoiseArgs);
MCA_MVDR_NOISE_PLAIN_TABLE(MCA_MVDR_MASK_NOISE_PLAIN_INST)
#undef MCA_MVDR_MASK_NOISE_PLAIN_INST
#define MCA_MVDR_MASK_NOISE_NULLS_INST(Q, S, S1, PF, R) template __global__ void k_mvdr_masked_t<Q, false, S, S1, PF && MCA_MVDR_MASK_PF(Q, S), true, false, true>(MvdrGateNoiseArgs);
MCA_MVDR_GATE_NULLS_TABLE(MCA_MVDR_MASK_NOISE_NULLS_INST)
#undef MCA_MVDR_MASK_NOISE_NULLS_INST

}  // namespace mca
