// kernels_mvdr_solve_frame_noise.hip -- the instantiations of k_mvdr_solve_t (mvdr_solve.h) with
// a weight per frame and the noise plane of the post-filter.
#include "mvdr_solve.h"

namespace mca {
template const void *mvdr_solve_kernel_of<MvdrWeight::FRAME, true>(int, bool, int, bool, int *);
}  // namespace mca
