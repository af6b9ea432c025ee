// mvdr_gate.h -- the template of the MVDR solve with a per-frame covariance update weight (gfx950; include/mcarray_hip.h,
// mca_hip_mvdr_sources_frames_weighted_dev), shared by the translation units that instantiate it:
// kernels_mvdr_gate.hip (k_mvdr_gated_t<..., NOISE = false>) and kernels_mvdr_gate_noise.hip (NOISE = true: the
// kernels of a call with the post-filter enabled), and kernels_mvdr_mask.hip / kernels_mvdr_mask_noise.hip for
// k_mvdr_masked_t, the same statements (mvdr_gate_body.h) with a weight per frame and bin.  The kernels have translation units and argument structs of their
// own, so that the unweighted kernels of kernels_mvdr.hip and kernels_mvdr_nulls.hip keep their code objects
// (kernels_mvdr_nulls.hip on why), and the kernels without the noise plane theirs beside those with it.
//
// Per stream a, bin and frame t, with u = fminf(fmaxf(update[a][t], 0), 1) (a NaN weight becomes 0):
//     a_t = 1 - (1 - alpha) u,  Phi_t = a_t Phi_{t-1} + (1 - a_t) x x^H,  tr_t = a_t tr_{t-1} + (1 - a_t) |x|^2
// u == 1 takes the context's own fp32 alpha and 1 - alpha and the operations of the unweighted kernels; u == 0 does not touch Phi
// and tr at all.  Everything behind the recursion is k_mvdr_solve / k_mvdr_solve_sources (NULLS = false) or k_mvdr_nulls
// (NULLS = true), operation for operation: one template serves the three, because k_mvdr_solve_sources already is k_mvdr_solve per
// look direction (S = 1 here) and k_mvdr_nulls is k_mvdr_solve_sources plus the Gram matrix of the directions.  Where those kernels
// leave the contraction of the loading into the pivot to the compiler, this one spells out what the compiler chose there.
//
// REUSE: a frame with u == 0 that follows a frame this workgroup has solved finds PhiL, and with it L and the inverse pivots, as
// that frame left them.  L lives in registers across the frame loop anyway; the inverse pivot of row j is kept by the lane that
// owns the row (Q more registers).  Such a frame runs only the forward substitutions of its columns (u = L^-1 d per direction,
// v = L^-1 x; the parked u of the nulls) -- the same operations in the same order on the same L bits as a frame that factorises, so
// its output does not depend on which of the two it did.  The first solved frame of a launch or of a piece always factorises.
//
// MASKED (k_mvdr_masked_t): the weight is update[(a F + t) K + k], one per problem and frame: the four lanes of a quad
// read one address, the 64 quads of a workgroup 64 consecutive floats.  frozen is then the quad's own and the recursion a
// divergent branch; every quad_bcast / quad_sum / __shfl_xor(.., 4) stays inside a quad, whose four lanes take the branch together
// (the silence branch has always been per quad).  The masked instantiations take REUSE = false (MCA_MVDR_MASK_* in mca_internal.h):
// the bits are those of the factorisation either way.
//
// NOISE: the lane that stores Y[(s F + t) K + k] also stores the residual noise power of the plain estimate of that direction,
// 1 / (d_s^H PhiL_t^-1 d_s), to pn at the same index (fp32) -- the reciprocal of den[s] that the output divides by (the plain
// den[s] = G_ss also under the nulls) -- and 0 for a bin that is digitally silent so far.  Like Y it is stored for t >= t_first only.
#pragma once
#include "fft_block.h"
#include "mca_internal.h"
#include "mvdr_nulls.h"
#include "mvdr_solve.h"

namespace mca {

// the kernel argument: MvdrGateArgs as it always was without the noise plane, MvdrGateNoiseArgs with it
__device__ __forceinline__ const MvdrGateArgs &mvdr_gate_args(const MvdrGateArgs &a) { return a; }
__device__ __forceinline__ const MvdrGateArgs &mvdr_gate_args(const MvdrGateNoiseArgs &a) { return a.g; }
__device__ __forceinline__ float *mvdr_noise_plane(const MvdrGateArgs &) { return nullptr; }
__device__ __forceinline__ float *mvdr_noise_plane(const MvdrGateNoiseArgs &a) { return a.pn; }

template <int Q, bool FULL, int S, int S1, bool PF, bool NULLS, bool REUSE, bool NOISE>
__global__ __launch_bounds__(256, 2) void k_mvdr_gated_t(MvdrGateArgsOf<NOISE> ka)
{
    constexpr bool MASKED = false;
#include "mvdr_gate_body.h"
}

// the same with a weight per (stream, frame, bin): MvdrGateArgs::update is update_mask[streams][n_frames][K]
// (mca_hip_mvdr_sources_frames_masked_dev; kernels_mvdr_mask.hip, kernels_mvdr_mask_noise.hip)
template <int Q, bool FULL, int S, int S1, bool PF, bool NULLS, bool REUSE, bool NOISE>
__global__ __launch_bounds__(256, 2) void k_mvdr_masked_t(MvdrGateArgsOf<NOISE> ka)
{
    constexpr bool MASKED = true;
#include "mvdr_gate_body.h"
}

}  // namespace mca
