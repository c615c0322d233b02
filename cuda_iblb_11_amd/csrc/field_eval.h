// field_eval.h — the per-sample evaluation shared by the readers: iblb_get_fields (field_kernels.hip),
// iblb_reduce_fields (reduce_kernels.hip), iblb_sample_points (tracer_kernels.hip) and iblb_set_average
// (average_kernels.hip) call the same device functions, so a sample has the same bits whether it is copied
// out, reduced, interpolated or accumulated on the device.  Contraction is off
// in every function: one rounding per operation.
#pragma once

#include "../../include/iblb.h"

#include "iblb_kernels.h"

namespace iblb {

// The nine populations f^t of cell (xc, y) as doubles (as pull_cell of lbm_kernels.hip)
template <typename T>
__device__ __forceinline__ void pull_cell(const T* g, const Layout& L, const Halo<T>& H, int xc, int y, double f[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = Store<T>::to_f(pull<T>(g, L, H, xc, y, k), k);
}

// rho, u and the populations of cell (xc, y) exactly as iblb_get_macro / iblb_get_populations
// return them: the arithmetic of macro_out_kernel (lbm_kernels.hip) in the run phase; in the boot
// phase the given rho^0, u^0 and the unstreamed f^0 in place (macro_device, pop_out_kernel(raw)).
template <typename T>
__device__ __forceinline__ void cell_state(const T* __restrict__ g, const Layout& L, const Halo<T>& H,
                                           const FieldsArgs& a, int xc, int y, double f[9], double& r, double& ux,
                                           double& uy) {
#pragma clang fp contract(off)
    const long o = (long)xc * L.rows + y;
    if (a.rho0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = Store<T>::to_f(g[k * L.plane + (long)xc * L.col + y], k);
        r = a.rho0[o];
        ux = a.u0[o];
        uy = a.u0[a.fplane + o];
        return;
    }
    pull_cell<T>(g, L, H, xc, y, f);
    double mx, my;
    moments<double>(f, r, mx, my);
    const double Fx = (a.fdense ? a.fdense[o] : 0.) + a.gx;
    const double Fy = (a.fdense ? a.fdense[a.fplane + o] : 0.) + a.gy;
    ux = (mx + 0.5 * Fx) / r;
    uy = (my + 0.5 * Fy) / r;
}

static_assert(FIELD_SCALAR_BITS == (IBLB_FIELD_C | IBLB_FIELD_CUX | IBLB_FIELD_CUY) &&
                  IBLB_FIELD_C == 1u << FIELD_SCALAR_BIT0 && IBLB_FIELD_CUX == 2u << FIELD_SCALAR_BIT0 &&
                  IBLB_FIELD_CUY == 4u << FIELD_SCALAR_BIT0,
              "FIELD_SCALAR_BITS mirrors include/iblb.h");

// A reader's kernel with the scalar's fields needs the fluid state of a cell unless IBLB_FIELD_C is all it was
// asked for (uniform over the launch); the builds without the scalar always do.
template <bool SCALAR>
__device__ __forceinline__ bool wants_fluid(const FieldsArgs& a) {
    return !SCALAR || (a.fields & ~(unsigned)IBLB_FIELD_C) != 0;
}

// C of cell (xc, y) exactly as iblb_get_scalar returns it (scalar_out_kernel of scalar_kernels.hip): the five
// stored populations summed in this order.  Lanes along y: each of the five loads is one contiguous run per wave.
__device__ __forceinline__ double cell_scalar(const FieldsArgs& a, int xc, int y) {
#pragma clang fp contract(off)
    const double* q = a.sc + (long)xc * a.sc_rows + y;
    return (((q[0] + q[a.sc_plane]) + q[2 * a.sc_plane]) + q[3 * a.sc_plane]) + q[4 * a.sc_plane];
}

// d(uy)/dx - d(ux)/dy at cell (xc, y) whose own u_x is ux: central differences at lattice spacing 1,
// periodic in x (the neighbour columns modulo ncol: a lone slab only); one-sided at the walls
template <typename T>
__device__ __forceinline__ double cell_vorticity(const T* __restrict__ g, const Layout& L, const Halo<T>& H,
                                                 const FieldsArgs& a, int xc, int y, double ux) {
#pragma clang fp contract(off)
    double fn[9], rn, uxa, uxb, uya, uyb, t;
    cell_state<T>(g, L, H, a, xc + 1 < L.ncol ? xc + 1 : 0, y, fn, rn, t, uyb);
    cell_state<T>(g, L, H, a, xc > 0 ? xc - 1 : L.ncol - 1, y, fn, rn, t, uya);
    const double duy_dx = (uyb - uya) / 2.0;
    double dux_dy;
    if (y == 0) {
        cell_state<T>(g, L, H, a, xc, 1, fn, rn, uxb, t);
        dux_dy = uxb - ux;
    } else if (y == L.ny - 1) {
        cell_state<T>(g, L, H, a, xc, y - 1, fn, rn, uxa, t);
        dux_dy = ux - uxa;
    } else {
        cell_state<T>(g, L, H, a, xc, y + 1, fn, rn, uxb, t);
        cell_state<T>(g, L, H, a, xc, y - 1, fn, rn, uxa, t);
        dux_dy = (uxb - uxa) / 2.0;
    }
    return duy_dx - dux_dy;
}

// Viscous stress kvisc * PiNeq, PiNeq = sum_i c_i c_i (f_i - feq_i(rho, u)), feq as
// LatticeBoltzmann.cu:45-49 in double
__device__ __forceinline__ void cell_stress(const double f[9], double r, double ux, double uy, double kvisc,
                                            double& sxx, double& sxy, double& syy) {
#pragma clang fp contract(off)
    constexpr double C_S = 0.57735;
    const double usq = (ux * ux + uy * uy) / (2 * C_S * C_S);
    double pxx = 0., pxy = 0., pyy = 0.;
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        const double cu = ux * cx(i) + uy * cy(i);
        const double feq = r * wgt(i) * (1 + cu / (C_S * C_S) + cu * cu / (2 * C_S * C_S * C_S * C_S) - usq);
        const double d = f[i] - feq;
        if (cx(i) != 0) pxx += d;
        if (cy(i) != 0) pyy += d;
        if (cx(i) * cy(i) > 0) pxy += d;
        if (cx(i) * cy(i) < 0) pxy -= d;
    }
    sxx = kvisc * pxx;
    sxy = kvisc * pxy;
    syy = kvisc * pyy;
}

}  // namespace iblb
