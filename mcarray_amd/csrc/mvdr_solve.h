// mvdr_solve.h -- what the MVDR solve kernels of kernels_mvdr.hip and kernels_mvdr_nulls.hip share: the quad broadcasts, the
// compile-time column loop and the steering vectors of a lane's rows.
#pragma once
#include "fft512.h"
#include "mca_internal.h"

#include <type_traits>

namespace mca {

template <int B>
__device__ __forceinline__ float quad_bcast1(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), B * 0x55, 0xf, 0xf, true));   // quad_perm:[B,B,B,B]
}
__device__ __forceinline__ float quad_bcast(float v, int b)
{
    switch (b) {
    case 0: return quad_bcast1<0>(v);
    case 1: return quad_bcast1<1>(v);
    case 2: return quad_bcast1<2>(v);
    default: return quad_bcast1<3>(v);
    }
}
__device__ __forceinline__ float2 quad_bcast(float2 v, int b) { return make_float2(quad_bcast(v.x, b), quad_bcast(v.y, b)); }

// f(integral_constant<int, J0>), ..., f(integral_constant<int, J1 - 1>): the column loop of the solve kernels written out at compile time.  As
// a "#pragma unroll" loop it passes the size up to which the compiler honours the pragma once a column carries three right-hand
// sides, and a loop left rolled puts L and P into scratch.
template <int J0, int J1, class Fn>
__device__ __forceinline__ void mvdr_static_for(Fn &&f)
{
    if constexpr (J0 < J1) {
        f(std::integral_constant<int, J0>{});
        mvdr_static_for<J0 + 1, J1>(f);
    }
}

// steering d_i of look direction s in frame t for the rows of this lane (T already offset to the stream and k >> 5)
template <int Q, bool FULL>
__device__ __forceinline__ void mvdr_steer_rows(float2 (&d)[Q], const float2 *T, long long ts, int M, int nph, int lo_off, int l)
{
    float2 th[Q], tl[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float2 *tq = T + (ts * M + ((FULL || 4 * q + l < M) ? 4 * q + l : 0)) * nph;
        th[q] = tq[0]; tl[q] = tq[lo_off];
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) d[q] = (FULL || 4 * q + l < M) ? cmul(th[q], tl[q]) : make_float2(0.f, 0.f);
}

}  // namespace mca
