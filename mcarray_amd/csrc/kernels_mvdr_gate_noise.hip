// kernels_mvdr_gate_noise.hip -- the gated MVDR solve that also emits the residual noise power of every output (gfx950;
// include/mcarray_hip.h, mca_hip_mvdr_set_postfilter): the NOISE = true instantiations of mvdr_gate.h, which every
// call of a context with the post-filter enabled takes (a call without update weights with a buffer of ones).  A translation
// unit and an argument struct of their own, so that the kernels without the noise plane keep their code objects.
#include "mvdr_gate.h"

namespace mca {

#define MCA_MVDR_NOISE_PLAIN_INST(Q, S, S1F, S1P, PFP, RF, RP)                                                  \
    template __global__ void k_mvdr_gated_t<Q, true, S, S1F, true, false, RF, true>(MvdrGateNoiseArgs);          \
    template __global__ void k_mvdr_gated_t<Q, false, S, S1P, PFP, false, RP, true>(MvdrGateNoiseArgs);
MCA_MVDR_NOISE_PLAIN_TABLE(MCA_MVDR_NOISE_PLAIN_INST)
#undef MCA_MVDR_NOISE_PLAIN_INST
#define MCA_MVDR_NOISE_NULLS_INST(Q, S, S1, PF, R) template __global__ void k_mvdr_gated_t<Q, false, S, S1, PF, true, R, true>(MvdrGateNoiseArgs);
MCA_MVDR_GATE_NULLS_TABLE(MCA_MVDR_NOISE_NULLS_INST)
#undef MCA_MVDR_NOISE_NULLS_INST

}  // namespace mca
