// skip_box.h — a patch output region of the IB band cycle, shared by the deep sweeps' arguments
// (iblb_kernels.h) and the host-only band planner (band_plan.h).  Standard C++ only.
#pragma once

namespace iblb {

// IB band cycle with its last level beside the deep sweep (and a group slab's boundary sweeps): a patch output region the
// last level stores and the deep sweep must not: local columns [x0, x1] (inclusive) x rows [y0, y1)
// (even bounds, so that a lane's two cells are both in or both out)
struct SkipBox {
    int x0, x1, y0, y1;
};
constexpr int MAX_SKIP = 96;

}  // namespace iblb
