// particle_kernels.hip — the tracers under a motion model (include/iblb.h iblb_set_tracer_model): particles that
// the flow carries, that jitter by a counter-based random step, settle with a drift and deposit on a wall.
//
// One lane = one tracer, as in tracer_kernels.hip: SoA positions read and written coalesced, the four cells of
// a tracer a gather of 36 population loads evaluated through point_eval.h, so the sampled velocity has the bits
// of tracer_advect_kernel's.  A lane reads its status first: a deposited tracer leaves before the gather.  The
// two random numbers of an update are two 64-bit integer hashes of (seed, tracer, update, component): no state,
// so a run cut into calls, restarted or re-based draws the same numbers.  No atomics and no cross-lane steps in
// the update; the per-column deposit counts are integer atomics, exact whatever the order of arrival.
#include "point_eval.h"

namespace iblb {

__device__ __forceinline__ unsigned long long particle_mix(unsigned long long z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// xi in [-1, 1), exact: 53 bits of the hash scaled by 2^-52
__device__ __forceinline__ double particle_xi(unsigned long long key, unsigned long long counter) {
#pragma clang fp contract(off)
    const unsigned long long r = particle_mix(key + 0x9E3779B97F4A7C15ull * counter);
    return (double)(r >> 11) * 0x1p-52 - 1.0;
}

// One update of the alive tracers with the state held fixed (include/iblb.h iblb_set_tracer_model, steps 1 to 5)
template <typename T>
__global__ __launch_bounds__(256) void particle_advect_kernel(const T* __restrict__ g, Layout L, Halo<T> H, FieldsArgs a,
                                                              long n, double stride, ParticleStep P,
                                                              double* __restrict__ x, double* __restrict__ y,
                                                              int* __restrict__ laps, int* __restrict__ status,
                                                              long long* __restrict__ hit) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (status[p] != IBLB_TRACER_ALIVE) return;  // deposited: it never moves again
    const double xp = x[p], yp = y[p];
    const Bilinear q = bilinear_of(xp, yp, L.ncol, L.ny);
    double f[9], r, ux00, uy00, ux10, uy10, ux01, uy01, ux11, uy11;
    cell_state<T>(g, L, H, a, q.i0, q.j0, f, r, ux00, uy00);
    cell_state<T>(g, L, H, a, q.i1, q.j0, f, r, ux10, uy10);
    cell_state<T>(g, L, H, a, q.i0, q.j1, f, r, ux01, uy01);
    cell_state<T>(g, L, H, a, q.i1, q.j1, f, r, ux11, uy11);
    const double ux = bilinear_mix(q, ux00, ux10, ux01, ux11);
    const double uy = bilinear_mix(q, uy00, uy10, uy01, uy11);
    if (!(isfinite(ux) && isfinite(uy))) return;  // the tracer keeps its position and stays alive
    const double X = (double)L.ncol, ytop = (double)(L.ny - 1);
    double xn = xp + stride * (ux + P.drift[0]), yn = yp + stride * (uy + P.drift[1]);
    if (P.amp != 0.) {
        const unsigned long long key = particle_mix(P.seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)p + 1ull));
        const unsigned long long c0 = 2ull * (unsigned long long)P.m + 1ull;
        xn = xn + P.amp * particle_xi(key, c0);
        yn = yn + P.amp * particle_xi(key, c0 + 1ull);
    }
    const bool low = yn < 0., high = yn > ytop;
    if (low || high) {
        const int kind = P.wall[low ? 0 : 1];
        const double yw = low ? 0. : ytop;
        if (kind == IBLB_TRACER_WALL_ABSORB) {
            const double lam = (yw - yp) / (yn - yp);
            xn = xp + lam * (xn - xp);
            yn = yw;
            status[p] = low ? IBLB_TRACER_AT_BOTTOM : IBLB_TRACER_AT_TOP;
            hit[p] = P.t;
        } else if (kind == IBLB_TRACER_WALL_REFLECT) {
            yn = low ? -yn : yw - (yn - yw);
            yn = yn < 0. ? 0. : (yn > ytop ? ytop : yn);
        } else {
            yn = yw;
        }
    }
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
    y[p] = yn;
}

// The deposited tracers per column floor(x) and wall: dep[i] bottom, dep[ncol + i] top
__global__ __launch_bounds__(256) void particle_deposit_kernel(long n, int ncol, const double* __restrict__ x,
                                                               const int* __restrict__ status,
                                                               unsigned long long* __restrict__ dep) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int st = status[p];
    if (st != IBLB_TRACER_AT_BOTTOM && st != IBLB_TRACER_AT_TOP) return;
    const double fx = floor(x[p]);
    const int i = fx >= 0. ? (fx < (double)ncol ? (int)fx : ncol - 1) : 0;  // (in range for every stored x)
    atomicAdd(dep + (st == IBLB_TRACER_AT_TOP ? ncol : 0) + i, 1ull);
}

template <typename T>
hipError_t launch_particle_advect(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, long n, int stride,
                                  const ParticleStep& P, double* x, double* y, int* laps, int* status, long long* hit,
                                  hipStream_t s) {
    if (n <= 0) return hipSuccess;
    particle_advect_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(g, L, H, a, n, (double)stride, P, x, y, laps,
                                                                         status, hit);
    return hipGetLastError();
}

hipError_t launch_particle_deposit(long n, int ncol, const double* x, const int* status, unsigned long long* dep,
                                   hipStream_t s) {
    hipError_t e = hipMemsetAsync(dep, 0, 2 * (size_t)ncol * sizeof(unsigned long long), s);
    if (e != hipSuccess || n <= 0) return e;
    particle_deposit_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, ncol, x, status, dep);
    return hipGetLastError();
}

template hipError_t launch_particle_advect<double>(const double*, Layout, Halo<double>, const FieldsArgs&, long, int,
                                                   const ParticleStep&, double*, double*, int*, int*, long long*,
                                                   hipStream_t);
template hipError_t launch_particle_advect<float>(const float*, Layout, Halo<float>, const FieldsArgs&, long, int,
                                                  const ParticleStep&, double*, double*, int*, int*, long long*,
                                                  hipStream_t);

}  // namespace iblb
