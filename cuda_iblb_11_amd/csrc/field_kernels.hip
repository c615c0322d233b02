// field_kernels.hip — the windowed field reader of iblb_get_fields (include/iblb.h): rho, u,
// vorticity and viscous stress on a strided window of the slab, written at the window's size.
//
// One lane = one sample.  Lanes run along the window's y: the populations are stored y-fastest and
// the loads (9 per sample, 45 with vorticity) outnumber the stores (one per selected field).  No
// atomics, no reductions: every output value is a function of its own cell (and, for vorticity, of
// its four neighbours).
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

template <typename T>
__global__ __launch_bounds__(256) void fields_out_kernel(const T* __restrict__ g, Layout L, Halo<T> H, FieldsArgs a,
                                                         double* __restrict__ out) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)a.nxl * a.nyw) return;
    const int il = (int)(idx / a.nyw), j = (int)(idx - (long)il * a.nyw);
    const int xc = a.xl0 + il * a.sx, y = a.y0 + j * a.sy;
    double f[9], r, ux, uy;
    cell_state<T>(g, L, H, a, xc, y, f, r, ux, uy);
    const long plane = (long)a.nyw * a.nxl;
    double* o = out + (long)j * a.nxl + il;
    if (a.fields & IBLB_FIELD_RHO) { *o = r; o += plane; }
    if (a.fields & IBLB_FIELD_UX) { *o = ux; o += plane; }
    if (a.fields & IBLB_FIELD_UY) { *o = uy; o += plane; }
    if (a.fields & IBLB_FIELD_VORT) {
        // central differences at lattice spacing 1, periodic in x; one-sided at the walls
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
        *o = duy_dx - dux_dy;
        o += plane;
    }
    if (a.fields & (IBLB_FIELD_SXX | IBLB_FIELD_SXY | IBLB_FIELD_SYY)) {
        // PiNeq = sum_i c_i c_i (f_i - feq_i(rho, u)), feq as LatticeBoltzmann.cu:45-49 in double
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
        if (a.fields & IBLB_FIELD_SXX) { *o = a.kvisc * pxx; o += plane; }
        if (a.fields & IBLB_FIELD_SXY) { *o = a.kvisc * pxy; o += plane; }
        if (a.fields & IBLB_FIELD_SYY) { *o = a.kvisc * pyy; o += plane; }
    }
}

template <typename T>
hipError_t launch_fields_out(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, double* out, hipStream_t s) {
    const long n = (long)a.nxl * a.nyw;
    if (n <= 0) return hipSuccess;
    fields_out_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(g, L, H, a, out);
    return hipGetLastError();
}

template hipError_t launch_fields_out<double>(const double*, Layout, Halo<double>, const FieldsArgs&, double*,
                                              hipStream_t);
template hipError_t launch_fields_out<float>(const float*, Layout, Halo<float>, const FieldsArgs&, double*, hipStream_t);

}  // namespace iblb
