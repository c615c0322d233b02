// tracer_kernels.hip — the Lagrangian side of the readers (include/iblb.h): bilinear sampling of the
// fields at arbitrary points (iblb_sample_points) and the explicit-Euler update of the context's passive
// tracers (iblb_set_tracers; launched by iblb_step at the update iterations).
//
// One lane = one point.  Lanes run along the point index: the positions are SoA doubles, read and
// written coalesced; the four cells of a point are a gather (9 population loads each, 45 with
// vorticity), served by the caches where neighbouring points share cells.  No atomics, no cross-lane
// steps: every output value is a function of its own point and the state.  Each of the four cells is
// evaluated by the device functions of field_eval.h, so a cell's value has the bits iblb_get_fields
// returns for it; the interpolation is the header's expression, one rounding per operation (both through
// point_eval.h, which the history recorder of history_kernels.hip shares).  With the scalar's
// fields a cell costs five more loads, and C*ux, C*uy are formed per cell before they are interpolated.
#include "point_eval.h"

namespace iblb {

// out[k*n + p]: the k-th set bit of a.fields at point p = (xy[p], xy[n + p]).  SCALAR: one of the scalar's
// fields is requested (FIELD_SCALAR_BITS); the build without carries none of their code.
template <typename T, bool SCALAR>
__global__ __launch_bounds__(256) void sample_points_kernel(const T* __restrict__ g, Layout L, Halo<T> H, FieldsArgs a,
                                                            long n, const double* __restrict__ xy,
                                                            double* __restrict__ out) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const Bilinear q = bilinear_of(xy[p], xy[n + p], L.ncol, L.ny);
    constexpr int NV = SCALAR ? 10 : 7;
    double v00[NV], v10[NV], v01[NV], v11[NV];
    cell_fields<T, SCALAR>(g, L, H, a, q.i0, q.j0, v00);
    cell_fields<T, SCALAR>(g, L, H, a, q.i1, q.j0, v10);
    cell_fields<T, SCALAR>(g, L, H, a, q.i0, q.j1, v01);
    cell_fields<T, SCALAR>(g, L, H, a, q.i1, q.j1, v11);
    double* o = out + p;
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (a.fields & (1u << (k < 7 ? k : k - 7 + FIELD_SCALAR_BIT0))) {
            *o = bilinear_mix(q, v00[k], v10[k], v01[k], v11[k]);
            o += n;
        }
}

// One explicit-Euler update of the tracers with the state held fixed (include/iblb.h iblb_set_tracers):
// x += stride * ux(x, y), y += stride * uy(x, y); x wraps periodically (laps counts the wraps), y is
// clamped to the walls' rows.  A stored position stays finite and in range.
template <typename T>
__global__ __launch_bounds__(256) void tracer_advect_kernel(const T* __restrict__ g, Layout L, Halo<T> H, FieldsArgs a,
                                                            long n, double stride, double* __restrict__ x,
                                                            double* __restrict__ y, int* __restrict__ laps) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double xp = x[p], yp = y[p];
    const Bilinear q = bilinear_of(xp, yp, L.ncol, L.ny);
    double f[9], r, ux00, uy00, ux10, uy10, ux01, uy01, ux11, uy11;
    cell_state<T>(g, L, H, a, q.i0, q.j0, f, r, ux00, uy00);
    cell_state<T>(g, L, H, a, q.i1, q.j0, f, r, ux10, uy10);
    cell_state<T>(g, L, H, a, q.i0, q.j1, f, r, ux01, uy01);
    cell_state<T>(g, L, H, a, q.i1, q.j1, f, r, ux11, uy11);
    const double ux = bilinear_mix(q, ux00, ux10, ux01, ux11);
    const double uy = bilinear_mix(q, uy00, uy10, uy01, uy11);
    if (!(isfinite(ux) && isfinite(uy))) return;  // the tracer keeps its position
    const double X = (double)L.ncol, ytop = (double)(L.ny - 1);
    double xn = xp + stride * ux, yn = yp + stride * uy;
    int lp = laps[p];
    if (xn >= X) {
        xn -= X;
        lp += 1;
    } else if (xn < 0.) {
        xn += X;
        lp -= 1;
    }
    if (xn >= 0. && xn < X) {  // else more than one lattice length in one update: x and laps stay
        x[p] = xn;
        laps[p] = lp;
    }
    yn = yn < 0. ? 0. : (yn > ytop ? ytop : yn);
    y[p] = yn;
}

template <typename T>
hipError_t launch_sample_points(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, long n, const double* xy,
                                double* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (a.fields & FIELD_SCALAR_BITS) {
        if (!a.sc) return hipErrorInvalidValue;
        sample_points_kernel<T, true><<<grid, 256, 0, s>>>(g, L, H, a, n, xy, out);
    } else {
        sample_points_kernel<T, false><<<grid, 256, 0, s>>>(g, L, H, a, n, xy, out);
    }
    return hipGetLastError();
}

template <typename T>
hipError_t launch_tracer_advect(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, long n, int stride, double* x,
                                double* y, int* laps, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    tracer_advect_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(g, L, H, a, n, (double)stride, x, y, laps);
    return hipGetLastError();
}

template hipError_t launch_sample_points<double>(const double*, Layout, Halo<double>, const FieldsArgs&, long,
                                                 const double*, double*, hipStream_t);
template hipError_t launch_sample_points<float>(const float*, Layout, Halo<float>, const FieldsArgs&, long, const double*,
                                                double*, hipStream_t);
template hipError_t launch_tracer_advect<double>(const double*, Layout, Halo<double>, const FieldsArgs&, long, int,
                                                 double*, double*, int*, hipStream_t);
template hipError_t launch_tracer_advect<float>(const float*, Layout, Halo<float>, const FieldsArgs&, long, int, double*,
                                                double*, int*, hipStream_t);

}  // namespace iblb
