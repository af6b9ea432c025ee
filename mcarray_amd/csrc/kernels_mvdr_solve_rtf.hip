// kernels_mvdr_solve_rtf.hip -- the instantiations of k_mvdr_solve_rtf_t (mvdr_solve.h): steering vectors from
// the plane of k_mvdr_rtf, a weight per frame and bin, without the noise plane of the post-filter.
#include "mvdr_solve.h"

namespace mca {
template const void *mvdr_solve_rtf_kernel_of<false>(int, bool, int);
}  // namespace mca
