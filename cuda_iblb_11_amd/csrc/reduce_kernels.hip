// reduce_kernels.hip — the window reduction of iblb_reduce_fields (include/iblb.h): count, sums,
// extrema with their locations, row sums and column sums of the chosen quantities over a strided
// window of the slab, without copying the window out.
//
// Pass 1: one lane = one window row, walking a chunk of the window's columns.  Lanes run along y (the
// populations are stored y-fastest: every load of a wave is one contiguous run), a sample is
// evaluated once (field_eval.h, the functions of iblb_get_fields) and feeds every requested quantity.
// The lane's running sum is its row's partial sum; a column's sum over the wave's 64 rows is a
// cross-lane butterfly per sample; the statistics of the workgroup come from one more butterfly per
// quantity and an LDS step over its four waves at the end.  Every partial goes to a place of its own
// in the scratch (ReduceGeom, iblb_kernels.h).  Pass 2, a separate launch, adds the partials in
// ascending index order.  No atomics, nothing depends on which workgroup runs first: the result is a
// function of the state and the window.
#include <algorithm>

#include "field_eval.h"

namespace iblb {

namespace {

constexpr int RS = REDUCE_RS;

__device__ __forceinline__ bool finite(double v) {
    return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}
// (v, i, j) before (w, wi, wj): the smaller value, at equal values the lower j, then the lower i
// (the first in row-major order, numpy's argmin); `bigger` the same for the larger value
__device__ __forceinline__ bool smaller(double v, int i, int j, double w, int wi, int wj) {
    return v < w || (v == w && (j < wj || (j == wj && i < wi)));
}
__device__ __forceinline__ bool bigger(double v, int i, int j, double w, int wi, int wj) {
    return v > w || (v == w && (j < wj || (j == wj && i < wi)));
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// one statistics record += another (both REDUCE_RS doubles; the empty record: 0, 0, 0, 0, +inf, -inf, -1 x 4)
__device__ __forceinline__ void merge_record(double* a, const double* b) {
#pragma clang fp contract(off)
    a[0] += b[0];
    a[1] += b[1];
    a[2] += b[2];
    a[3] += b[3];
    if (smaller(b[4], (int)b[6], (int)b[7], a[4], (int)a[6], (int)a[7])) a[4] = b[4], a[6] = b[6], a[7] = b[7];
    if (bigger(b[5], (int)b[8], (int)b[9], a[5], (int)a[8], (int)a[9])) a[5] = b[5], a[8] = b[8], a[9] = b[9];
}
__device__ __forceinline__ void empty_record(double* a) {
    a[0] = a[1] = a[2] = a[3] = 0.;
    a[4] = __builtin_inf();
    a[5] = -__builtin_inf();
    a[6] = a[7] = a[8] = a[9] = -1.;
}

// HEAVY: vorticity or a stress component is requested (bits 3 .. 6); the light build carries neither
// their code nor their accumulators.  SCALAR: one of the scalar's quantities is requested (bits 12 .. 14,
// quantities 11 .. 13 here); the builds without carry neither their code nor their accumulators.
template <typename T, bool HEAVY, bool SCALAR>
__global__ __launch_bounds__(REDUCE_ROWS) void reduce_pass1_kernel(const T* __restrict__ g, Layout L, Halo<T> H,
                                                                   FieldsArgs a, ReduceGeom q,
                                                                   double* __restrict__ scratch) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rbi = blockIdx.x, cbi = blockIdx.y;
    const int j = rbi * REDUCE_ROWS + tid;
    // lanes past the window's last row evaluate that row again (in bounds) and contribute nothing:
    // every lane takes part in every cross-lane step
    const bool valid = j < a.nyw;
    const int y = a.y0 + (valid ? j : a.nyw - 1) * a.sy;
    const int il0 = cbi * q.cc, il1 = min(a.nxl, il0 + q.cc);
    const unsigned fields = a.fields;
    constexpr int NQ = SCALAR ? REDUCE_NQ + 3 : REDUCE_NQ;
    auto bit = [](int k) { return k < REDUCE_NQ ? k : k - REDUCE_NQ + FIELD_SCALAR_BIT0; };  // quantity k's bit
    auto wanted = [&](int k) { return (HEAVY || k < 3 || k > 6) && ((fields >> bit(k)) & 1u); };
    // the place of quantity k in the output: the set bits below its own (ascending bit order)
    auto slot = [&](int k) { return __builtin_popcount(fields & ((1u << bit(k)) - 1u)); };

    double sum[NQ], sq[NQ], mn[NQ], mx[NQ];
    int bad[NQ], mni[NQ], mxi[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        sum[k] = sq[k] = 0.;
        mn[k] = __builtin_inf();
        mx[k] = -__builtin_inf();
        bad[k] = 0;
        mni[k] = mxi[k] = -1;
    }
    double* colp = scratch + q.o_col + (long)(rbi * (REDUCE_ROWS / 64) + wave) * q.nf * a.nxl;

    for (int il = il0; il < il1; ++il) {
        const int xc = a.xl0 + il * a.sx;
        double f[9], v[NQ];
#pragma unroll
        for (int k = 0; k < NQ; ++k) v[k] = 0.;
        if (wants_fluid<SCALAR>(a)) cell_state<T>(g, L, H, a, xc, y, f, v[0], v[1], v[2]);
        const double r = v[0], ux = v[1], uy = v[2];
        if constexpr (SCALAR) {
            v[REDUCE_NQ] = cell_scalar(a, xc, y);
            v[REDUCE_NQ + 1] = v[REDUCE_NQ] * ux;
            v[REDUCE_NQ + 2] = v[REDUCE_NQ] * uy;
        }
        if constexpr (HEAVY) {
            if (fields & IBLB_FIELD_VORT) v[3] = cell_vorticity<T>(g, L, H, a, xc, y, ux);
            if (fields & (IBLB_FIELD_SXX | IBLB_FIELD_SXY | IBLB_FIELD_SYY))
                cell_stress(f, r, ux, uy, a.kvisc, v[4], v[5], v[6]);
        }
        const double usq = ux * ux + uy * uy;
        v[7] = r * ux;
        v[8] = r * uy;
        v[9] = 0.5 * (r * usq);
        v[10] = usq;
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            if (!wanted(k)) continue;
            const bool fin = valid && finite(v[k]);
            const double x = fin ? v[k] : 0.;  // a skipped sample adds an exact zero
            bad[k] += valid && !fin;
            sum[k] += x;
            sq[k] += x * x;
            if (fin && v[k] < mn[k]) mn[k] = v[k], mni[k] = il;  // strict: the lowest i of the row stays
            if (fin && v[k] > mx[k]) mx[k] = v[k], mxi[k] = il;
            if (q.cols) {
                const double c = wave_sum(x);
                if (lane == 0) colp[(long)slot(k) * a.nxl + il] = c;
            }
        }
    }

    __shared__ double red[REDUCE_ROWS / 64][NQ][RS];
    const int nvalid = valid ? il1 - il0 : 0;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        if (!wanted(k)) continue;
        if (q.rows && valid) scratch[q.o_row + ((long)cbi * q.nf + slot(k)) * a.nyw + j] = sum[k];
        const int nbad = wave_sum_int(bad[k]);
        const int cnt = wave_sum_int(nvalid - bad[k]);
        const double s = wave_sum(sum[k]), s2 = wave_sum(sq[k]);
        double lo = mn[k], hi = mx[k];
        int loi = mni[k], loj = mni[k] < 0 ? -1 : j, hii = mxi[k], hij = mxi[k] < 0 ? -1 : j;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double w = __shfl_xor(lo, o, 64);
            const int wi = __shfl_xor(loi, o, 64), wj = __shfl_xor(loj, o, 64);
            if (smaller(w, wi, wj, lo, loi, loj)) lo = w, loi = wi, loj = wj;
            const double z = __shfl_xor(hi, o, 64);
            const int zi = __shfl_xor(hii, o, 64), zj = __shfl_xor(hij, o, 64);
            if (bigger(z, zi, zj, hi, hii, hij)) hi = z, hii = zi, hij = zj;
        }
        if (lane == 0) {
            double* p = red[wave][k];
            p[0] = cnt, p[1] = nbad, p[2] = s, p[3] = s2, p[4] = lo, p[5] = hi;
            p[6] = loi < 0 ? -1 : q.i_first + loi, p[7] = loj;
            p[8] = hii < 0 ? -1 : q.i_first + hii, p[9] = hij;
        }
    }
    __syncthreads();
    if (tid < NQ && wanted(tid)) {
        double rec[RS];
        empty_record(rec);
        for (int w = 0; w < REDUCE_ROWS / 64; ++w) merge_record(rec, red[w][tid]);
        double* out = scratch + ((long)(cbi * q.rb + rbi) * q.nf + slot(tid)) * RS;
        for (int e = 0; e < RS; ++e) out[e] = rec[e];
    }
}

// Pass 2.  Workgroup b < nf: the statistics of quantity b over every pass-1 workgroup: lane t merges the
// records t, t + 256, ... in that order, then the 256 lanes' records are merged pairwise through LDS
// (t with t + 128, then t + 64, ...): a fixed tree for a given number of records.  The workgroups after
// them: one lane per (quantity, row) adds the column chunks' partial row sums in ascending chunk order,
// then one lane per (quantity, x) the waves' partial column sums in ascending row order.
__global__ __launch_bounds__(256) void reduce_pass2_kernel(ReduceGeom q, int nxl, int nyw, double* __restrict__ scratch) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, b = blockIdx.x;
    double* out = scratch + q.o_out;
    if (b < q.nf) {
        __shared__ double tree[256][RS];
        double rec[RS];
        empty_record(rec);
        const int nwg = q.cb * q.rb;
        for (int w = tid; w < nwg; w += 256) merge_record(rec, scratch + ((long)w * q.nf + b) * RS);
        for (int e = 0; e < RS; ++e) tree[tid][e] = rec[e];
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) merge_record(tree[tid], tree[tid + s]);
            __syncthreads();
        }
        if (tid < RS) out[(long)b * RS + tid] = tree[0][tid];
        return;
    }
    const long nrow = q.rows ? (long)q.nf * nyw : 0, ncol = q.cols ? (long)q.nf * nxl : 0;
    const long idx = (long)(b - q.nf) * 256 + tid;
    if (idx < nrow) {
        double s = 0.;
        for (int c = 0; c < q.cb; ++c) s += scratch[q.o_row + (long)c * nrow + idx];
        out[(long)q.nf * RS + idx] = s;
    } else if (idx - nrow < ncol) {
        const long e = idx - nrow;
        double s = 0.;
        for (int w = 0; w < q.rb * (REDUCE_ROWS / 64); ++w) s += scratch[q.o_col + (long)w * ncol + e];
        out[(long)q.nf * RS + nrow + e] = s;
    }
}

}  // namespace

// Column chunks: enough workgroups to fill the device (about 1024 of four waves), at least 8 columns
// each so that a lane amortises its set-up, at most 128 chunks so that the row partials stay a small
// fraction of the window.
ReduceGeom reduce_geometry(int nxl, int nyw, int nf, bool rows, bool cols) {
    ReduceGeom q{};
    q.rb = (nyw + REDUCE_ROWS - 1) / REDUCE_ROWS;
    const int want = std::min(128, std::max(1, (1024 + q.rb - 1) / q.rb));
    q.cc = std::max(8, (nxl + want - 1) / want);
    q.cb = (nxl + q.cc - 1) / q.cc;
    q.nf = nf;
    q.rows = rows;
    q.cols = cols;
    q.o_row = (long)q.cb * q.rb * nf * RS;
    q.o_col = q.o_row + (rows ? (long)q.cb * nf * nyw : 0);
    q.o_out = q.o_col + (cols ? (long)q.rb * (REDUCE_ROWS / 64) * nf * nxl : 0);
    q.n_out = (long)nf * RS + (rows ? (long)nf * nyw : 0) + (cols ? (long)nf * nxl : 0);
    q.n_scratch = q.o_out + q.n_out;
    return q;
}

template <typename T>
hipError_t launch_reduce_fields(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, const ReduceGeom& q,
                                double* scratch, hipStream_t s) {
    if (a.nxl <= 0 || a.nyw <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)q.rb, (unsigned)q.cb);
    const bool heavy = a.fields & (IBLB_FIELD_VORT | IBLB_FIELD_SXX | IBLB_FIELD_SXY | IBLB_FIELD_SYY);
    const bool scalar = a.fields & FIELD_SCALAR_BITS;
    if (scalar && !a.sc) return hipErrorInvalidValue;
    if (heavy && scalar) reduce_pass1_kernel<T, true, true><<<grid, REDUCE_ROWS, 0, s>>>(g, L, H, a, q, scratch);
    else if (heavy) reduce_pass1_kernel<T, true, false><<<grid, REDUCE_ROWS, 0, s>>>(g, L, H, a, q, scratch);
    else if (scalar) reduce_pass1_kernel<T, false, true><<<grid, REDUCE_ROWS, 0, s>>>(g, L, H, a, q, scratch);
    else reduce_pass1_kernel<T, false, false><<<grid, REDUCE_ROWS, 0, s>>>(g, L, H, a, q, scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long tail = (q.n_out - (long)q.nf * RS + 255) / 256;
    reduce_pass2_kernel<<<(unsigned)(q.nf + tail), 256, 0, s>>>(q, a.nxl, a.nyw, scratch);
    return hipGetLastError();
}

template hipError_t launch_reduce_fields<double>(const double*, Layout, Halo<double>, const FieldsArgs&,
                                                 const ReduceGeom&, double*, hipStream_t);
template hipError_t launch_reduce_fields<float>(const float*, Layout, Halo<float>, const FieldsArgs&,
                                                const ReduceGeom&, double*, hipStream_t);

}  // namespace iblb
