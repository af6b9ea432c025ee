// kernels_mvdr_solve_rtf_nulls_noise.hip -- the instantiations of k_mvdr_solve_rtf_nulls_t (mvdr_solve.h) that also store the
// noise plane of the post-filter.
#include "mvdr_solve.h"

namespace mca {
template const void *mvdr_solve_rtf_nulls_kernel_of<true>(int, int, int *);
}  // namespace mca
