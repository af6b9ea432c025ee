// kernels_mvdr_solve_rtf_nulls.hip -- the instantiations of k_mvdr_solve_rtf_nulls_t (mvdr_solve.h): soft nulls at the steering
// vectors of the plane of k_mvdr_rtf, without the noise plane of the post-filter.
#include "mvdr_solve.h"

namespace mca {
template const void *mvdr_solve_rtf_nulls_kernel_of<false>(int, int, int *);
}  // namespace mca
