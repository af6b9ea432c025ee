// kernels_mvdr_solve_cell.hip -- the instantiations of k_mvdr_solve_t (mvdr_solve.h) with
// a covariance update weight per frame and bin (mca_hip_mvdr_sources_frames_masked_*).
#include "mvdr_solve.h"

namespace mca {
template const void *mvdr_solve_kernel_of<MvdrWeight::CELL, false>(int, bool, int, bool, int *);
}  // namespace mca
