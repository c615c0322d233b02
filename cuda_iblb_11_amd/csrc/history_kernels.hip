// history_kernels.hip — the recorder of iblb_set_history (include/iblb.h): one record of the probes' samples
// appended to a ring on the device, and the per-probe running statistics beside it, in one launch at the
// record iterations of iblb_step.
//
// One lane = one probe.  Lanes run along the probe index: the positions are SoA doubles (the history's own
// copy, or the context's tracers under FOLLOW), read coalesced; the four cells of a probe are the gather of
// sample_points_kernel (tracer_kernels.hip), evaluated by the same device functions (point_eval.h), so a
// recorded value has the bits iblb_sample_points returns for that position.  A record is np planes of n
// doubles, plane k at slot[k*n + p]: every plane is written as coalesced runs along p.  The statistics are
// eight arrays of np*n entries at the same index; an entry has one writer per record (its probe's lane) and
// the records are ordered by the stream, so there are no atomics and no cross-lane steps, and the totals are
// reproducible bit for bit.  Contraction is off: one rounding per operation.
#include "point_eval.h"

namespace iblb {

// One value v of record m folded into entry e of the statistics (include/iblb.h iblb_set_history)
__device__ __forceinline__ void history_fold(const HistoryStats& s, long e, double v, long long m) {
#pragma clang fp contract(off)
    if (!isfinite(v)) {
        s.nonfinite[e] += 1;
        return;
    }
    s.count[e] += 1;
    s.sum[e] = s.sum[e] + v;
    s.sum_sq[e] = s.sum_sq[e] + v * v;
    if (v < s.min[e]) {
        s.min[e] = v;
        s.min_rec[e] = m;
    }
    if (v > s.max[e]) {
        s.max[e] = v;
        s.max_rec[e] = m;
    }
}

// Record m of n probes into `slot` ([np][n]) and into the statistics.  FOLLOW: the probes are the tracers
// (x, y, laps), and the record starts with the planes x, y, (double)laps; a.fields may then be 0.  SCALAR: one
// of the scalar's fields is requested (FIELD_SCALAR_BITS); the builds without carry none of their code.
template <typename T, bool SCALAR, bool FOLLOW>
__global__ __launch_bounds__(256) void history_record_kernel(const T* __restrict__ g, Layout L, Halo<T> H, FieldsArgs a,
                                                             long n, const double* __restrict__ x,
                                                             const double* __restrict__ y, const int* __restrict__ laps,
                                                             long long m, double* __restrict__ slot, HistoryStats s) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double xp = x[p], yp = y[p];
    long e = p;
    if constexpr (FOLLOW) {
        const double lead[3] = {xp, yp, (double)laps[p]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            slot[e] = lead[k];
            history_fold(s, e, lead[k], m);
            e += n;
        }
        if (!a.fields) return;  // positions only (uniform over the launch)
    }
    const Bilinear q = bilinear_of(xp, yp, L.ncol, L.ny);
    constexpr int NV = SCALAR ? 10 : 7;
    double v00[NV], v10[NV], v01[NV], v11[NV];
    cell_fields<T, SCALAR>(g, L, H, a, q.i0, q.j0, v00);
    cell_fields<T, SCALAR>(g, L, H, a, q.i1, q.j0, v10);
    cell_fields<T, SCALAR>(g, L, H, a, q.i0, q.j1, v01);
    cell_fields<T, SCALAR>(g, L, H, a, q.i1, q.j1, v11);
#pragma unroll
    for (int k = 0; k < NV; ++k)
        if (a.fields & (1u << (k < 7 ? k : k - 7 + FIELD_SCALAR_BIT0))) {
            const double v = bilinear_mix(q, v00[k], v10[k], v01[k], v11[k]);
            slot[e] = v;
            history_fold(s, e, v, m);
            e += n;
        }
}

template <typename T>
hipError_t launch_history_record(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, long n, const double* x,
                                 const double* y, const int* laps, long long m, double* slot, const HistoryStats& s,
                                 hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!laps && !a.fields) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + 255) / 256);
    const bool scalar = (a.fields & FIELD_SCALAR_BITS) != 0;
    if (scalar && !a.sc) return hipErrorInvalidValue;
    if (laps) {
        if (scalar) history_record_kernel<T, true, true><<<grid, 256, 0, st>>>(g, L, H, a, n, x, y, laps, m, slot, s);
        else history_record_kernel<T, false, true><<<grid, 256, 0, st>>>(g, L, H, a, n, x, y, laps, m, slot, s);
    } else {
        if (scalar) history_record_kernel<T, true, false><<<grid, 256, 0, st>>>(g, L, H, a, n, x, y, laps, m, slot, s);
        else history_record_kernel<T, false, false><<<grid, 256, 0, st>>>(g, L, H, a, n, x, y, laps, m, slot, s);
    }
    return hipGetLastError();
}

template hipError_t launch_history_record<double>(const double*, Layout, Halo<double>, const FieldsArgs&, long,
                                                  const double*, const double*, const int*, long long, double*,
                                                  const HistoryStats&, hipStream_t);
template hipError_t launch_history_record<float>(const float*, Layout, Halo<float>, const FieldsArgs&, long, const double*,
                                                 const double*, const int*, long long, double*, const HistoryStats&,
                                                 hipStream_t);

}  // namespace iblb
