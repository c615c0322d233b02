// average_kernels.hip — time- and phase-averaged fields (include/iblb.h iblb_set_average): the
// accumulate kernel iblb_step launches at the sample iterations, and the read-out kernel of
// iblb_get_average.
//
// Accumulate: one lane = one window sample, lanes along the window's y (the populations are stored
// y-fastest: the nine loads of a sample are one contiguous run per wave).  A sample is evaluated once
// by the device functions of field_eval.h, so its value has the bits iblb_get_fields returns for it,
// and is then added into the current bin's accumulator planes with a read-modify-write.  The planes
// are kept in the order the lanes run, [plane][il * nyw + j], so that both halves of the
// read-modify-write coalesce.  Every accumulator element belongs to exactly one lane: no atomics, no
// cross-lane steps, and the sums are a function of the samples and their order alone.  Contraction
// is off: sum + v, sum_sq + v*v and sum_uxuy + ux*uy round once per operation.
//
// Read-out: a tiled transpose through LDS of the planes of one bin into the layout of the ABI,
// [plane][j * nxl + il], so that the host copies whole planes.
#include "field_eval.h"

namespace iblb {

namespace {

constexpr int TILE = 32;  // read-out: TILE x TILE elements per workgroup of TILE x 8 lanes

// HEAVY: vorticity or a stress component is requested (bits 3 .. 6); the light build carries none of
// their code.  SCALAR: one of the scalar's fields is requested (FIELD_SCALAR_BITS): five more loads per sample,
// one contiguous run per wave each like the fluid's nine; the builds without carry none of that code.
template <typename T, bool HEAVY, bool SCALAR>
__global__ __launch_bounds__(256) void average_accum_kernel(const T* __restrict__ g, Layout L, Halo<T> H, FieldsArgs a,
                                                            unsigned flags, double* __restrict__ acc) {
#pragma clang fp contract(off)
    const long n = (long)a.nxl * a.nyw;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int il = (int)(idx / a.nyw), j = (int)(idx - (long)il * a.nyw);
    // the host validated the window against the lattice; the cell indices are clamped all the same, so
    // that no window, whatever its values, forms an index outside the buffers
    const int xc = min(max(a.xl0 + il * a.sx, 0), L.ncol - 1), y = min(max(a.y0 + j * a.sy, 0), L.ny - 1);
    double f[9], v[7];
#pragma unroll
    for (int k = SCALAR ? 0 : 3; k < 7; ++k) v[k] = 0.;
    if (wants_fluid<SCALAR>(a)) cell_state<T>(g, L, H, a, xc, y, f, v[0], v[1], v[2]);
    const double ux = v[1], uy = v[2];
    if constexpr (HEAVY) {
        if (a.fields & IBLB_FIELD_VORT) v[3] = cell_vorticity<T>(g, L, H, a, xc, y, ux);
        if (a.fields & (IBLB_FIELD_SXX | IBLB_FIELD_SXY | IBLB_FIELD_SYY))
            cell_stress(f, v[0], ux, uy, a.kvisc, v[4], v[5], v[6]);
    }
    // planes of a bin: nf sums, then nf sums of squares (IBLB_AVG_SQ), then one of ux*uy (IBLB_AVG_UXUY)
    const int nf = __builtin_popcount(a.fields);
    const bool sq = flags & IBLB_AVG_SQ;
    double* p = acc + idx;
#pragma unroll
    for (int k = 0; k < (HEAVY ? 7 : 3); ++k) {
        if (!((a.fields >> k) & 1u)) continue;
        *p = *p + v[k];
        if (sq) {
            double* q = p + (long)nf * n;
            *q = *q + v[k] * v[k];
        }
        p += n;
    }
    if constexpr (SCALAR) {
        const double c = cell_scalar(a, xc, y);
        const double vs[3] = {c, c * ux, c * uy};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!((a.fields >> (FIELD_SCALAR_BIT0 + k)) & 1u)) continue;
            *p = *p + vs[k];
            if (sq) {
                double* q = p + (long)nf * n;
                *q = *q + vs[k] * vs[k];
            }
            p += n;
        }
    }
    if (flags & IBLB_AVG_UXUY) {
        double* q = acc + (long)(sq ? 2 * nf : nf) * n + idx;
        *q = *q + ux * uy;
    }
}

// out[(p * nyw + j) * nxl + il] = acc[(p * nxl + il) * nyw + j] for the planes p < gridDim.z
__global__ __launch_bounds__(TILE * 8) void average_readout_kernel(const double* __restrict__ acc, int nxl, int nyw,
                                                                   double* __restrict__ out) {
    __shared__ double tile[TILE][TILE + 1];
    const long plane = (long)nxl * nyw;
    const double* src = acc + blockIdx.z * plane;
    double* dst = out + blockIdx.z * plane;
    const int j0 = blockIdx.x * TILE, i0 = blockIdx.y * TILE;
    for (int r = threadIdx.y; r < TILE; r += 8) {  // rows of the tile along il, lanes along j
        const int il = i0 + r, j = j0 + threadIdx.x;
        if (il < nxl && j < nyw) tile[r][threadIdx.x] = src[(long)il * nyw + j];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < TILE; r += 8) {  // rows of the tile along j, lanes along il
        const int j = j0 + r, il = i0 + threadIdx.x;
        if (il < nxl && j < nyw) dst[(long)j * nxl + il] = tile[threadIdx.x][r];
    }
}

}  // namespace

template <typename T>
hipError_t launch_average_accum(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, unsigned flags, double* acc,
                                hipStream_t s) {
    const long n = (long)a.nxl * a.nyw;
    if (n <= 0) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + 255) / 256);
    const bool heavy = a.fields & (IBLB_FIELD_VORT | IBLB_FIELD_SXX | IBLB_FIELD_SXY | IBLB_FIELD_SYY);
    const bool scalar = a.fields & FIELD_SCALAR_BITS;
    if (scalar && !a.sc) return hipErrorInvalidValue;
    if (heavy && scalar) average_accum_kernel<T, true, true><<<grid, 256, 0, s>>>(g, L, H, a, flags, acc);
    else if (heavy) average_accum_kernel<T, true, false><<<grid, 256, 0, s>>>(g, L, H, a, flags, acc);
    else if (scalar) average_accum_kernel<T, false, true><<<grid, 256, 0, s>>>(g, L, H, a, flags, acc);
    else average_accum_kernel<T, false, false><<<grid, 256, 0, s>>>(g, L, H, a, flags, acc);
    return hipGetLastError();
}

hipError_t launch_average_readout(const double* acc, int nxl, int nyw, int planes, double* out, hipStream_t s) {
    if (nxl <= 0 || nyw <= 0 || planes <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((nyw + TILE - 1) / TILE), (unsigned)((nxl + TILE - 1) / TILE), (unsigned)planes);
    average_readout_kernel<<<grid, dim3(TILE, 8), 0, s>>>(acc, nxl, nyw, out);
    return hipGetLastError();
}

template hipError_t launch_average_accum<double>(const double*, Layout, Halo<double>, const FieldsArgs&, unsigned,
                                                 double*, hipStream_t);
template hipError_t launch_average_accum<float>(const float*, Layout, Halo<float>, const FieldsArgs&, unsigned, double*,
                                                hipStream_t);

}  // namespace iblb
