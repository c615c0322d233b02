// field_kernels.hip — the windowed field reader of iblb_get_fields (include/iblb.h): rho, u,
// vorticity, viscous stress and the passive scalar's C, C*ux, C*uy on a strided window of the slab,
// written at the window's size.
//
// One lane = one sample.  Lanes run along the window's y: the populations are stored y-fastest and
// the loads (9 per sample, 45 with vorticity, 5 more with the scalar) outnumber the stores (one per
// selected field).  No atomics, no reductions: every output value is a function of its own cell (and,
// for vorticity, of its four neighbours).
#include "field_eval.h"

namespace iblb {

// SCALAR: one of the scalar's fields is requested (FIELD_SCALAR_BITS); the build without carries none of
// their code.
template <typename T, bool SCALAR>
__global__ __launch_bounds__(256) void fields_out_kernel(const T* __restrict__ g, Layout L, Halo<T> H, FieldsArgs a,
                                                         double* __restrict__ out) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)a.nxl * a.nyw) return;
    const int il = (int)(idx / a.nyw), j = (int)(idx - (long)il * a.nyw);
    const int xc = a.xl0 + il * a.sx, y = a.y0 + j * a.sy;
    double f[9], r = 0., ux = 0., uy = 0.;
    if (wants_fluid<SCALAR>(a)) cell_state<T>(g, L, H, a, xc, y, f, r, ux, uy);
    const long plane = (long)a.nyw * a.nxl;
    double* o = out + (long)j * a.nxl + il;
    if (a.fields & IBLB_FIELD_RHO) { *o = r; o += plane; }
    if (a.fields & IBLB_FIELD_UX) { *o = ux; o += plane; }
    if (a.fields & IBLB_FIELD_UY) { *o = uy; o += plane; }
    if (a.fields & IBLB_FIELD_VORT) {
        *o = cell_vorticity<T>(g, L, H, a, xc, y, ux);
        o += plane;
    }
    if (a.fields & (IBLB_FIELD_SXX | IBLB_FIELD_SXY | IBLB_FIELD_SYY)) {
        double sxx, sxy, syy;
        cell_stress(f, r, ux, uy, a.kvisc, sxx, sxy, syy);
        if (a.fields & IBLB_FIELD_SXX) { *o = sxx; o += plane; }
        if (a.fields & IBLB_FIELD_SXY) { *o = sxy; o += plane; }
        if (a.fields & IBLB_FIELD_SYY) { *o = syy; o += plane; }
    }
    if constexpr (SCALAR) {
        const double c = cell_scalar(a, xc, y);
        if (a.fields & IBLB_FIELD_C) { *o = c; o += plane; }
        if (a.fields & IBLB_FIELD_CUX) { *o = c * ux; o += plane; }
        if (a.fields & IBLB_FIELD_CUY) { *o = c * uy; o += plane; }
    }
}

template <typename T>
hipError_t launch_fields_out(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, double* out, hipStream_t s) {
    const long n = (long)a.nxl * a.nyw;
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (a.fields & FIELD_SCALAR_BITS) {
        if (!a.sc) return hipErrorInvalidValue;
        fields_out_kernel<T, true><<<grid, 256, 0, s>>>(g, L, H, a, out);
    } else {
        fields_out_kernel<T, false><<<grid, 256, 0, s>>>(g, L, H, a, out);
    }
    return hipGetLastError();
}

template hipError_t launch_fields_out<double>(const double*, Layout, Halo<double>, const FieldsArgs&, double*,
                                              hipStream_t);
template hipError_t launch_fields_out<float>(const float*, Layout, Halo<float>, const FieldsArgs&, double*, hipStream_t);

}  // namespace iblb
