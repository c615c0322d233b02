// lbm_sweepk6.hip — the K = 6 iterations-per-launch sweeps (sweepk_kernel, lbm_sweep_impl.h),
// one translation unit per depth so that the deep kernels build in parallel.
#include "lbm_sweep_impl.h"

IBLB_SWEEPK_UNIT(6)
