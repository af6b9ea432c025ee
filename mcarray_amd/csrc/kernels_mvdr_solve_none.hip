// kernels_mvdr_solve_none.hip -- the instantiations of k_mvdr_solve_t (mvdr_solve.h) with
// no covariance update weights: the sources and nulls calls (the single-look call keeps k_mvdr_solve of kernels_mvdr.hip).
#include "mvdr_solve.h"

namespace mca {
template const void *mvdr_solve_kernel_of<MvdrWeight::NONE, false>(int, bool, int, bool, int *);
}  // namespace mca
