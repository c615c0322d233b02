// point_eval.h — the evaluation of one off-lattice point shared by iblb_sample_points, the passive tracers
// (tracer_kernels.hip) and the history recorder (history_kernels.hip): the four cells and two weights of a
// position, the fields of one cell, and the bilinear mix.  One definition, so a recorded sample has the bits
// iblb_sample_points returns for that position.  Each cell is evaluated by the device functions of
// field_eval.h; contraction is off in every function: one rounding per operation.
#pragma once

#include "field_eval.h"

namespace iblb {

// The four cells and the two weights of a position (include/iblb.h iblb_sample_points).  The host
// validates every position it copies in and the update rule stores only positions in range; the
// indices are clamped to the lattice all the same, so that no position, whatever its value, forms an
// index outside the buffers (for a position in range the clamps change nothing).
struct Bilinear {
    int i0, i1, j0, j1;
    double a, b;
};

__device__ __forceinline__ Bilinear bilinear_of(double x, double y, int ncol, int ny) {
#pragma clang fp contract(off)
    Bilinear q;
    const double fx = floor(x), fy = floor(y);
    int i0 = fx >= 0. ? (fx < (double)ncol ? (int)fx : ncol - 1) : 0;  // (a NaN compares false: column 0)
    int j0 = fy >= 0. ? (fy < (double)(ny - 1) ? (int)fy : ny - 2) : 0;
    q.i0 = i0;
    q.i1 = i0 + 1 < ncol ? i0 + 1 : 0;
    q.j0 = j0;
    q.j1 = j0 + 1;
    q.a = x - fx;
    q.b = y - (double)j0;
    return q;
}

__device__ __forceinline__ double bilinear_mix(const Bilinear& q, double v00, double v10, double v01, double v11) {
#pragma clang fp contract(off)
    return (1.0 - q.b) * ((1.0 - q.a) * v00 + q.a * v10) + q.b * ((1.0 - q.a) * v01 + q.a * v11);
}

// The selected fields of cell (xc, y), in the order of the IBLB_FIELD_* bits, as fields_out_kernel
// (field_kernels.hip) evaluates them; SCALAR: then C, C*ux, C*uy (v[7 .. 9])
template <typename T, bool SCALAR>
__device__ __forceinline__ void cell_fields(const T* __restrict__ g, const Layout& L, const Halo<T>& H,
                                            const FieldsArgs& a, int xc, int y, double* v) {
#pragma clang fp contract(off)
    double f[9], r = 0., ux = 0., uy = 0.;
    if (wants_fluid<SCALAR>(a)) cell_state<T>(g, L, H, a, xc, y, f, r, ux, uy);
    if constexpr (SCALAR) {
        v[7] = cell_scalar(a, xc, y);
        v[8] = v[7] * ux;
        v[9] = v[7] * uy;
    }
    v[0] = r;
    v[1] = ux;
    v[2] = uy;
    v[3] = (a.fields & IBLB_FIELD_VORT) ? cell_vorticity<T>(g, L, H, a, xc, y, ux) : 0.;
    v[4] = v[5] = v[6] = 0.;
    if (a.fields & (IBLB_FIELD_SXX | IBLB_FIELD_SXY | IBLB_FIELD_SYY)) cell_stress(f, r, ux, uy, a.kvisc, v[4], v[5], v[6]);
}

}  // namespace iblb
