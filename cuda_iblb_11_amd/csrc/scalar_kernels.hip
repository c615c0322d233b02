// scalar_kernels.hip — the passive scalar (include/iblb.h iblb_set_scalar): a D2Q5 BGK advection-diffusion
// lattice for one concentration C that iblb_step advances at its event iterations with the fluid velocity of
// that moment held fixed.
//
// Layout.  Five planes of ncol * rows doubles, s[i * plane + x * rows + y] (rows = ny rounded up to whole waves,
// as the dense force): y fastest, one lane per cell, lanes along y, so every load and store of a wave is one
// contiguous run.  Two such buffers (ping-pong) and a two-plane scratch for ux, uy in the same order.
//
// Substep: PUSH form.  A lane loads the five populations and the velocity of its own cell (7 planes), relaxes,
// and stores p_i to the cell the direction points at, plane i (5 planes): 96 bytes per cell.  The streaming map
// with the wall rules is a bijection of (cell, direction): the population that would leave through a wall goes
// to the same cell's opposite direction instead, whose own source cell does not exist.  Every destination
// element has exactly one writer: no atomics, no cross-lane steps.  The stores along y land one row up / down:
// still one contiguous run per wave, shifted by 8 bytes.
// The first substep of an event evaluates (ux, uy) with cell_state of field_eval.h, so its bits are those of
// iblb_get_fields, and leaves them in the scratch; the later substeps read the scratch, not the nine populations.
// Contraction is off everywhere: one rounding per operation, as the rule of include/iblb.h states it.
// With a source (iblb_set_scalar_source) the SOURCE builds of the substep run: one more plane loaded, s(x, y) in the
// same layout, 104 bytes per cell; the lanes of rows 0 and ny - 1 also load their column's wall entry from one
// 4 * ncol array (the flux or the value, by the wall's kind).  Every term of the rule is evaluated: what the call
// left NULL is an array of zeros (or of the uniform wall value) on the device.  Without a source the builds
// without SOURCE run: the kernels as they were.
// With an uptake (iblb_set_scalar_uptake) the UPTAKE builds run: the lanes of rows 0 and ny - 1 also load their
// column's coefficient a and running total from the uptake's arrays ([2 * ncol] each) and store the total and the
// substep's net amount: four more 8-byte accesses per wall lane, a column stride apart like those of
// scalar_wall_flux_kernel, 2 / ny of a substep's traffic.  Every entry has one writer per substep (with ny == 1 one
// lane writes both walls' entries) and successive substeps are ordered by the stream: no atomics, and the sums are
// bit-reproducible.  Without an uptake the builds without UPTAKE run: the kernels as they were.
// With open ends (iblb_set_scalar_ends) the ENDS builds run: x does not wrap.  The lanes of column 0 store what
// g_1'(0, y) receives by the left end's kind instead of pushing p_2 to column ncol - 1, those of column ncol - 1
// likewise for g_2' and p_1: the map stays a bijection of (cell, direction), and with D2Q5 an end rule and a wall
// rule never concern the same direction.  x = blockIdx.x, so the end test is uniform over the workgroup.  An end lane
// loads its row's value and running total from the ends' arrays ([2 * ny] each, index k * ny + y) and stores the
// total and the substep's net amount: these accesses run along y with the lanes, contiguous like the planes'.  One
// writer per entry per substep (with ncol == 1 one lane writes both ends' entries), no atomics.  Without ends the
// builds without ENDS run: the kernels as they were.
// With gauges (iblb_set_scalar_gauges) the GAUGES builds run.  A lane holds exactly the p_i that cross the four links
// of its cell, so it adds p_1 to `right` of the station at its own column and p_2 to `left` of the station at the
// column to its left, p_3 to `up` of the level at its own row and p_4 to `down` of the level at the row below.  Which
// entries those are comes from two small index arrays, G.col[x] (x = blockIdx.x: one uniform 8-byte load per
// workgroup) and G.row[y] (one 8-byte load per lane, contiguous along y, 16 bytes per row for the whole launch to
// share); -1 means no gauge.  The station totals run along y with the lanes, contiguous like the ends'; the level
// totals are a column stride apart like the uptake's.  A read, an add and a store per gauged lane and link, ordinary
// vector stores, one writer per entry per substep, no atomics; no population is changed.  Under ENDS nothing crosses
// the link right of column ncol - 1: a station there adds 0.0, which changes no value, so its lanes skip it.  Without
// gauges the builds without GAUGES run: the kernels as they were.
//
// The transposes between the ABI's layouts ([y * nx + x]) and the device's go through an LDS tile so that both
// sides coalesce.
#include "field_eval.h"

namespace iblb {

namespace {

constexpr int TILE = 32;  // transposes: TILE x TILE elements per workgroup of TILE x 8 lanes
constexpr double SW0 = 1.0 / 3.0, SW1 = 1.0 / 6.0;

// One wall lane's store under an uptake (include/iblb.h iblb_set_scalar_uptake).  q: the population that would leave
// through the wall; e: the column's entry of the rule in force (the flux at a no-flux wall, the value at a _VALUE
// wall; without a source 0.0 and the uniform value); w: the column's index into the uptake's arrays.  Returns what
// the opposite direction of the same cell receives, and adds the net amount that entered to the column's total.
__device__ __forceinline__ double uptake_wall(double q, double e, bool value, const ScalarUptake& U, long w) {
#pragma clang fp contract(off)
    double out, net;
    if (value) {
        out = (2.0 * SW1) * e - q;
        net = out - q;
    } else {
        const double l = U.a[w] * q;
        out = (q - l) + e;
        net = e - l;
    }
    U.total[w] = U.total[w] + net;
    U.last[w] = net;
    return out;
}

// One end lane's store under open ends (include/iblb.h iblb_set_scalar_ends).  q: the population that would leave
// through end k; own: the cell's relaxed population of the opposite direction (what its inner neighbour receives);
// w: the row's index into the ends' arrays.  Returns what the opposite direction of the same cell receives, and adds
// the net amount that entered to the row's total.
__device__ __forceinline__ double end_cell(double q, double own, const ScalarEnds& E, int k, long w) {
#pragma clang fp contract(off)
    double out = q;
    if (E.kind[k] == IBLB_SCALAR_END_VALUE) out = (2.0 * SW1) * E.value[w] - q;
    else if (E.kind[k] == IBLB_SCALAR_END_OUTFLOW) out = own;
    const double net = out - q;
    E.total[w] = E.total[w] + net;
    E.last[w] = net;
    return out;
}

// One cell of a substep: g[5] of cell (x, y) relaxed towards the equilibrium at (ux, uy) and pushed into dst.
// SOURCE: the rule of iblb_set_scalar_source.  sv = s(x, y) of the lane's cell; the lanes of rows 0 and ny - 1 load
// their column's one wall entry (the flux or the value, by the wall's kind) from Q.walls.
// UPTAKE: the rule of iblb_set_scalar_uptake at those two rows, with or without a source.
// ENDS: the rule of iblb_set_scalar_ends at columns 0 and ncol - 1 for the directions 1 and 2; nothing wraps.
// GAUGES: the totals of iblb_set_scalar_gauges; p itself goes where it went.
template <bool SOURCE, bool UPTAKE, bool ENDS, bool GAUGES>
__device__ __forceinline__ void scalar_push(const double g[5], double ux, double uy, const ScalarGeom& S,
                                            const ScalarRule& R, const ScalarSource& Q, const ScalarUptake& U,
                                            const ScalarEnds& E, const ScalarGauges& G, double sv, int x, int y,
                                            double* __restrict__ dst) {
#pragma clang fp contract(off)
    const double C = (((g[0] + g[1]) + g[2]) + g[3]) + g[4];
    const double a[5] = {0.0, ux, -ux, uy, -uy};
    double p[5];
    double r = 0.0;
    if constexpr (SOURCE) {
        const double m = Q.decay * C;
        r = sv - m;
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double geq = ((i == 0 ? SW0 : SW1) * C) * (1.0 + 3.0 * a[i]);
        p[i] = g[i] - R.omega * (g[i] - geq);
        if constexpr (SOURCE) p[i] = p[i] + (i == 0 ? SW0 : SW1) * r;
    }
    const long o = (long)x * S.rows + y;
    if constexpr (GAUGES) {
        const int2 kc = G.col[x], kr = G.row[y];
        // (ENDS: no link right of column ncol - 1; kc.y of column 0 names the station there)
        if (kc.x >= 0 && !(ENDS && x + 1 >= S.ncol)) {
            const long w = (long)kc.x * S.ny + y;
            G.right[w] = G.right[w] + p[1];
        }
        if (kc.y >= 0 && !(ENDS && x == 0)) {
            const long w = (long)kc.y * S.ny + y;
            G.left[w] = G.left[w] + p[2];
        }
        if (kr.x >= 0) {
            const long w = (long)kr.x * S.ncol + x;
            G.up[w] = G.up[w] + p[3];
        }
        if (kr.y >= 0) {
            const long w = (long)kr.y * S.ncol + x;
            G.down[w] = G.down[w] + p[4];
        }
    }
    dst[o] = p[0];
    if constexpr (ENDS) {
        if (x + 1 < S.ncol) dst[S.plane + o + S.rows] = p[1];
        else dst[2 * S.plane + o] = end_cell(p[1], p[2], E, 1, (long)S.ny + y);
        if (x > 0) dst[2 * S.plane + o - S.rows] = p[2];
        else dst[S.plane + o] = end_cell(p[2], p[1], E, 0, (long)y);
    } else {
        const long oxp = (long)(x + 1 < S.ncol ? x + 1 : 0) * S.rows + y;
        const long oxm = (long)(x > 0 ? x - 1 : S.ncol - 1) * S.rows + y;
        dst[S.plane + oxp] = p[1];
        dst[2 * S.plane + oxm] = p[2];
    }
    if constexpr (UPTAKE) {
        if (y + 1 < S.ny) dst[3 * S.plane + o + 1] = p[3];
        else {
            const bool value = R.wall_kind[1] == IBLB_SCALAR_WALL_VALUE;
            double e = value ? R.wall_value[1] : 0.0;
            if constexpr (SOURCE) e = Q.walls[(long)(value ? 3 : 1) * S.ncol + x];
            dst[4 * S.plane + o] = uptake_wall(p[3], e, value, U, (long)S.ncol + x);
        }
        if (y > 0) dst[4 * S.plane + o - 1] = p[4];
        else {
            const bool value = R.wall_kind[0] == IBLB_SCALAR_WALL_VALUE;
            double e = value ? R.wall_value[0] : 0.0;
            if constexpr (SOURCE) e = Q.walls[(long)(value ? 2 : 0) * S.ncol + x];
            dst[3 * S.plane + o] = uptake_wall(p[4], e, value, U, (long)x);
        }
    } else if constexpr (SOURCE) {
        if (y + 1 < S.ny) dst[3 * S.plane + o + 1] = p[3];
        else {
            const bool value = R.wall_kind[1] == IBLB_SCALAR_WALL_VALUE;
            const double e = Q.walls[(long)(value ? 3 : 1) * S.ncol + x];
            dst[4 * S.plane + o] = value ? (2.0 * SW1) * e - p[3] : p[3] + e;
        }
        if (y > 0) dst[4 * S.plane + o - 1] = p[4];
        else {
            const bool value = R.wall_kind[0] == IBLB_SCALAR_WALL_VALUE;
            const double e = Q.walls[(long)(value ? 2 : 0) * S.ncol + x];
            dst[3 * S.plane + o] = value ? (2.0 * SW1) * e - p[4] : p[4] + e;
        }
    } else {
        if (y + 1 < S.ny) dst[3 * S.plane + o + 1] = p[3];
        else dst[4 * S.plane + o] = R.wall_kind[1] == IBLB_SCALAR_WALL_VALUE ? (2.0 * SW1) * R.wall_value[1] - p[3] : p[3];
        if (y > 0) dst[4 * S.plane + o - 1] = p[4];
        else dst[3 * S.plane + o] = R.wall_kind[0] == IBLB_SCALAR_WALL_VALUE ? (2.0 * SW1) * R.wall_value[0] - p[4] : p[4];
    }
}

// grid: (ncol, ceil(ny / 256)); one lane per cell.  The SOURCE builds load one more plane, Q.field; the others
// never touch Q.  U, then E, then G stand last: the builds without UPTAKE / ENDS / GAUGES never touch them, and their
// other arguments keep their places.
template <typename T, bool SOURCE, bool UPTAKE, bool ENDS, bool GAUGES>
__global__ __launch_bounds__(256) void scalar_first_kernel(const T* __restrict__ f, Layout L, Halo<T> H, FieldsArgs a,
                                                           ScalarGeom S, ScalarRule R, ScalarSource Q,
                                                           const double* __restrict__ src, double* __restrict__ dst,
                                                           double* __restrict__ uv, ScalarUptake U, ScalarEnds E,
                                                           ScalarGauges G) {
    const int x = blockIdx.x, y = blockIdx.y * 256 + threadIdx.x;
    if (x >= S.ncol || y >= S.ny) return;
    const long o = (long)x * S.rows + y;
    double g[5], pop[9], r, ux, uy, sv = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) g[i] = src[i * S.plane + o];
    if constexpr (SOURCE) sv = Q.field[o];
    cell_state<T>(f, L, H, a, x, y, pop, r, ux, uy);
    uv[o] = ux;
    uv[S.plane + o] = uy;
    scalar_push<SOURCE, UPTAKE, ENDS, GAUGES>(g, ux, uy, S, R, Q, U, E, G, sv, x, y, dst);
}

template <bool SOURCE, bool UPTAKE, bool ENDS, bool GAUGES>
__global__ __launch_bounds__(256) void scalar_next_kernel(ScalarGeom S, ScalarRule R, ScalarSource Q,
                                                          const double* __restrict__ src, double* __restrict__ dst,
                                                          const double* __restrict__ uv, ScalarUptake U,
                                                          ScalarEnds E, ScalarGauges G) {
    const int x = blockIdx.x, y = blockIdx.y * 256 + threadIdx.x;
    if (x >= S.ncol || y >= S.ny) return;
    const long o = (long)x * S.rows + y;
    double g[5], sv = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) g[i] = src[i * S.plane + o];
    if constexpr (SOURCE) sv = Q.field[o];
    scalar_push<SOURCE, UPTAKE, ENDS, GAUGES>(g, uv[o], uv[S.plane + o], S, R, Q, U, E, G, sv, x, y, dst);
}

// The equilibrium of C = c[x * rows + y] (device layout: plane 0 of dst's own transposed input) at the cell's
// velocity, into the five planes of dst; c may be plane 0 of dst (a lane reads its element before it writes it)
template <typename T>
__global__ __launch_bounds__(256) void scalar_init_kernel(const T* __restrict__ f, Layout L, Halo<T> H, FieldsArgs a,
                                                          ScalarGeom S, const double* c, double* dst) {
#pragma clang fp contract(off)
    const int x = blockIdx.x, y = blockIdx.y * 256 + threadIdx.x;
    if (x >= S.ncol || y >= S.ny) return;
    const long o = (long)x * S.rows + y;
    double pop[9], r, ux, uy;
    cell_state<T>(f, L, H, a, x, y, pop, r, ux, uy);
    const double C = c[o];
    const double av[5] = {0.0, ux, -ux, uy, -uy};
#pragma unroll
    for (int i = 0; i < 5; ++i) dst[i * S.plane + o] = ((i == 0 ? SW0 : SW1) * C) * (1.0 + 3.0 * av[i]);
}

// dev[p * plane + x * rows + y] = ref[p * ncol * ny + y * ncol + x] for the planes p < gridDim.z
__global__ __launch_bounds__(TILE * 8) void scalar_in_kernel(const double* __restrict__ ref, ScalarGeom S,
                                                             double* __restrict__ dev) {
    __shared__ double tile[TILE][TILE + 1];
    const double* src = ref + blockIdx.z * ((long)S.ncol * S.ny);
    double* dst = dev + blockIdx.z * S.plane;
    const int y0 = blockIdx.x * TILE, x0 = blockIdx.y * TILE;
    for (int r = threadIdx.y; r < TILE; r += 8) {  // rows of the tile along y, lanes along x
        const int y = y0 + r, x = x0 + threadIdx.x;
        if (x < S.ncol && y < S.ny) tile[r][threadIdx.x] = src[(long)y * S.ncol + x];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < TILE; r += 8) {  // rows of the tile along x, lanes along y
        const int x = x0 + r, y = y0 + threadIdx.x;
        if (x < S.ncol && y < S.ny) dst[(long)x * S.rows + y] = tile[threadIdx.x][r];
    }
}

// SUM false: out[p * nxw * nyw + j * nxw + i] = dev[p * plane + X * rows + Y] for the planes p < gridDim.z;
// SUM true:  out[j * nxw + i] = (((g0 + g1) + g2) + g3) + g4 of cell (X, Y);  X = x0 + i sx, Y = y0 + j sy
template <bool SUM>
__global__ __launch_bounds__(TILE * 8) void scalar_out_kernel(const double* __restrict__ dev, ScalarGeom S, int x0,
                                                              int y0, int nxw, int nyw, int sx, int sy,
                                                              double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double tile[TILE][TILE + 1];
    const double* src = dev + (SUM ? 0 : blockIdx.z * S.plane);
    double* dst = out + (SUM ? 0 : blockIdx.z * ((long)nxw * nyw));
    const int j0 = blockIdx.x * TILE, i0 = blockIdx.y * TILE;
    for (int r = threadIdx.y; r < TILE; r += 8) {  // rows of the tile along i, lanes along j
        const int i = i0 + r, j = j0 + threadIdx.x;
        if (i < nxw && j < nyw) {
            // the host validated the window; the cell is clamped all the same (as the field kernels do)
            const int x = min(max(x0 + i * sx, 0), S.ncol - 1), y = min(max(y0 + j * sy, 0), S.ny - 1);
            const double* q = src + (long)x * S.rows + y;
            tile[r][threadIdx.x] = SUM ? (((q[0] + q[S.plane]) + q[2 * S.plane]) + q[3 * S.plane]) + q[4 * S.plane] : q[0];
        }
    }
    __syncthreads();
    for (int r = threadIdx.y; r < TILE; r += 8) {  // rows of the tile along j, lanes along i
        const int j = j0 + r, i = i0 + threadIdx.x;
        if (i < nxw && j < nyw) dst[(long)j * nxw + i] = tile[threadIdx.x][r];
    }
}

// The wall flux of the last substep (include/iblb.h iblb_get_scalar_wall_flux): one lane per column, which reads
// row 0 of plane 3 and row ny - 1 of plane 4 (2 * ncol loads a column stride apart: nothing to coalesce, and a
// thousandth of a substep's traffic).  out[x]: the wall below row 0; out[ncol + x]: the wall above the top row.
// SOURCE: a no-flux wall returns the source's wall_flux entry, a _VALUE wall takes the source's wall_value entry.
template <bool SOURCE>
__global__ __launch_bounds__(256) void scalar_wall_flux_kernel(const double* __restrict__ dev, ScalarGeom S, ScalarRule R,
                                                               ScalarSource Q, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= S.ncol) return;
    const double g3 = dev[3 * S.plane + (long)x * S.rows], g4 = dev[4 * S.plane + (long)x * S.rows + (S.ny - 1)];
    if constexpr (SOURCE) {
        const bool v0 = R.wall_kind[0] == IBLB_SCALAR_WALL_VALUE, v1 = R.wall_kind[1] == IBLB_SCALAR_WALL_VALUE;
        const double e0 = Q.walls[(long)(v0 ? 2 : 0) * S.ncol + x], e1 = Q.walls[(long)(v1 ? 3 : 1) * S.ncol + x];
        out[x] = v0 ? 2.0 * g3 - (2.0 * SW1) * e0 : e0;
        out[S.ncol + x] = v1 ? 2.0 * g4 - (2.0 * SW1) * e1 : e1;
    } else {
        out[x] = R.wall_kind[0] == IBLB_SCALAR_WALL_VALUE ? 2.0 * g3 - (2.0 * SW1) * R.wall_value[0] : 0.0;
        out[S.ncol + x] = R.wall_kind[1] == IBLB_SCALAR_WALL_VALUE ? 2.0 * g4 - (2.0 * SW1) * R.wall_value[1] : 0.0;
    }
}

inline bool geom_ok(const ScalarGeom& S) {
    return S.ncol > 0 && S.ny > 0 && S.rows >= S.ny && S.plane >= (long)S.ncol * S.rows;
}
// a source has both of its arrays or neither
inline bool source_ok(const ScalarSource& Q) { return (Q.field != nullptr) == (Q.walls != nullptr); }
// an uptake has all three of its arrays or none
inline bool uptake_ok(const ScalarUptake& U) {
    return (U.a != nullptr) == (U.total != nullptr) && (U.a != nullptr) == (U.last != nullptr);
}
// open ends have all three of their arrays or none, and kinds among the three
inline bool ends_ok(const ScalarEnds& E) {
    if ((E.value != nullptr) != (E.total != nullptr) || (E.value != nullptr) != (E.last != nullptr)) return false;
    if (!E.value) return true;
    for (int k = 0; k < 2; ++k)
        if (E.kind[k] < IBLB_SCALAR_END_NOFLUX || E.kind[k] > IBLB_SCALAR_END_OUTFLOW) return false;
    return true;
}
// gauges have all six of their arrays or none
inline bool gauges_ok(const ScalarGauges& G) {
    const bool on = G.col != nullptr;
    return (G.row != nullptr) == on && (G.right != nullptr) == on && (G.left != nullptr) == on &&
           (G.up != nullptr) == on && (G.down != nullptr) == on;
}
inline dim3 cell_grid(const ScalarGeom& S) { return dim3((unsigned)S.ncol, (unsigned)((S.ny + 255) / 256)); }
inline dim3 tile_grid(int nx, int ny, int planes) {
    return dim3((unsigned)((ny + TILE - 1) / TILE), (unsigned)((nx + TILE - 1) / TILE), (unsigned)planes);
}

// the GAUGES build or the one without, by G.col, under the SOURCE, UPTAKE and ENDS the caller chose
template <typename T, bool SOURCE, bool UPTAKE, bool ENDS>
void first_launch_ends(dim3 grid, hipStream_t s, const T* f, Layout L, Halo<T> H, const FieldsArgs& a, ScalarGeom S,
                       ScalarRule R, ScalarSource Q, const double* src, double* dst, double* uv, ScalarUptake U,
                       ScalarEnds E, ScalarGauges G) {
    if (G.col)
        scalar_first_kernel<T, SOURCE, UPTAKE, ENDS, true><<<grid, 256, 0, s>>>(f, L, H, a, S, R, Q, src, dst, uv, U, E, G);
    else
        scalar_first_kernel<T, SOURCE, UPTAKE, ENDS, false><<<grid, 256, 0, s>>>(f, L, H, a, S, R, Q, src, dst, uv, U, E, G);
}

template <bool SOURCE, bool UPTAKE, bool ENDS>
void next_launch_ends(dim3 grid, hipStream_t s, ScalarGeom S, ScalarRule R, ScalarSource Q, const double* src,
                      double* dst, const double* uv, ScalarUptake U, ScalarEnds E, ScalarGauges G) {
    if (G.col) scalar_next_kernel<SOURCE, UPTAKE, ENDS, true><<<grid, 256, 0, s>>>(S, R, Q, src, dst, uv, U, E, G);
    else scalar_next_kernel<SOURCE, UPTAKE, ENDS, false><<<grid, 256, 0, s>>>(S, R, Q, src, dst, uv, U, E, G);
}

// the ENDS build or the one without, by E.value, under the SOURCE and UPTAKE the caller chose
template <typename T, bool SOURCE, bool UPTAKE>
void first_launch(dim3 grid, hipStream_t s, const T* f, Layout L, Halo<T> H, const FieldsArgs& a, ScalarGeom S,
                  ScalarRule R, ScalarSource Q, const double* src, double* dst, double* uv, ScalarUptake U,
                  ScalarEnds E, ScalarGauges G) {
    if (E.value) first_launch_ends<T, SOURCE, UPTAKE, true>(grid, s, f, L, H, a, S, R, Q, src, dst, uv, U, E, G);
    else first_launch_ends<T, SOURCE, UPTAKE, false>(grid, s, f, L, H, a, S, R, Q, src, dst, uv, U, E, G);
}

template <bool SOURCE, bool UPTAKE>
void next_launch(dim3 grid, hipStream_t s, ScalarGeom S, ScalarRule R, ScalarSource Q, const double* src, double* dst,
                 const double* uv, ScalarUptake U, ScalarEnds E, ScalarGauges G) {
    if (E.value) next_launch_ends<SOURCE, UPTAKE, true>(grid, s, S, R, Q, src, dst, uv, U, E, G);
    else next_launch_ends<SOURCE, UPTAKE, false>(grid, s, S, R, Q, src, dst, uv, U, E, G);
}

}  // namespace

template <typename T>
hipError_t launch_scalar_first(const T* f, Layout L, Halo<T> H, const FieldsArgs& a, ScalarGeom S, ScalarRule R,
                               ScalarSource Q, ScalarUptake U, ScalarEnds E, ScalarGauges G, const double* src,
                               double* dst, double* uv, hipStream_t s) {
    if (!geom_ok(S) || S.ncol != L.ncol || S.ny != L.ny || !source_ok(Q) || !uptake_ok(U) || !ends_ok(E) ||
        !gauges_ok(G))
        return hipErrorInvalidValue;
    const dim3 grid = cell_grid(S);
    if (U.a) {
        if (Q.field) first_launch<T, true, true>(grid, s, f, L, H, a, S, R, Q, src, dst, uv, U, E, G);
        else first_launch<T, false, true>(grid, s, f, L, H, a, S, R, Q, src, dst, uv, U, E, G);
    } else {
        if (Q.field) first_launch<T, true, false>(grid, s, f, L, H, a, S, R, Q, src, dst, uv, U, E, G);
        else first_launch<T, false, false>(grid, s, f, L, H, a, S, R, Q, src, dst, uv, U, E, G);
    }
    return hipGetLastError();
}

hipError_t launch_scalar_next(ScalarGeom S, ScalarRule R, ScalarSource Q, ScalarUptake U, ScalarEnds E, ScalarGauges G,
                              const double* src, double* dst, const double* uv, hipStream_t s) {
    if (!geom_ok(S) || !source_ok(Q) || !uptake_ok(U) || !ends_ok(E) || !gauges_ok(G)) return hipErrorInvalidValue;
    const dim3 grid = cell_grid(S);
    if (U.a) {
        if (Q.field) next_launch<true, true>(grid, s, S, R, Q, src, dst, uv, U, E, G);
        else next_launch<false, true>(grid, s, S, R, Q, src, dst, uv, U, E, G);
    } else {
        if (Q.field) next_launch<true, false>(grid, s, S, R, Q, src, dst, uv, U, E, G);
        else next_launch<false, false>(grid, s, S, R, Q, src, dst, uv, U, E, G);
    }
    return hipGetLastError();
}

template <typename T>
hipError_t launch_scalar_init(const T* f, Layout L, Halo<T> H, const FieldsArgs& a, ScalarGeom S, const double* c,
                              double* dst, hipStream_t s) {
    if (!geom_ok(S) || S.ncol != L.ncol || S.ny != L.ny) return hipErrorInvalidValue;
    scalar_init_kernel<T><<<cell_grid(S), 256, 0, s>>>(f, L, H, a, S, c, dst);
    return hipGetLastError();
}

hipError_t launch_scalar_in(const double* ref, ScalarGeom S, int planes, double* dev, hipStream_t s) {
    if (!geom_ok(S) || planes < 1 || planes > 5) return hipErrorInvalidValue;
    scalar_in_kernel<<<tile_grid(S.ncol, S.ny, planes), dim3(TILE, 8), 0, s>>>(ref, S, dev);
    return hipGetLastError();
}

hipError_t launch_scalar_populations_out(const double* dev, ScalarGeom S, double* out, hipStream_t s) {
    if (!geom_ok(S)) return hipErrorInvalidValue;
    scalar_out_kernel<false><<<tile_grid(S.ncol, S.ny, 5), dim3(TILE, 8), 0, s>>>(dev, S, 0, 0, S.ncol, S.ny, 1, 1, out);
    return hipGetLastError();
}

hipError_t launch_scalar_out(const double* dev, ScalarGeom S, int x0, int y0, int nxw, int nyw, int sx, int sy,
                             double* out, hipStream_t s) {
    if (!geom_ok(S) || nxw < 1 || nyw < 1) return hipErrorInvalidValue;
    scalar_out_kernel<true><<<tile_grid(nxw, nyw, 1), dim3(TILE, 8), 0, s>>>(dev, S, x0, y0, nxw, nyw, sx, sy, out);
    return hipGetLastError();
}

hipError_t launch_scalar_wall_flux(const double* dev, ScalarGeom S, ScalarRule R, ScalarSource Q, double* out,
                                   hipStream_t s) {
    if (!geom_ok(S) || !source_ok(Q)) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((S.ncol + 255) / 256);
    if (Q.field) scalar_wall_flux_kernel<true><<<blocks, 256, 0, s>>>(dev, S, R, Q, out);
    else scalar_wall_flux_kernel<false><<<blocks, 256, 0, s>>>(dev, S, R, Q, out);
    return hipGetLastError();
}

hipError_t launch_scalar_plane_out(const double* dev, ScalarGeom S, double* out, hipStream_t s) {
    if (!geom_ok(S)) return hipErrorInvalidValue;
    scalar_out_kernel<false><<<tile_grid(S.ncol, S.ny, 1), dim3(TILE, 8), 0, s>>>(dev, S, 0, 0, S.ncol, S.ny, 1, 1, out);
    return hipGetLastError();
}

template hipError_t launch_scalar_first<double>(const double*, Layout, Halo<double>, const FieldsArgs&, ScalarGeom,
                                                ScalarRule, ScalarSource, ScalarUptake, ScalarEnds, ScalarGauges,
                                                const double*, double*, double*, hipStream_t);
template hipError_t launch_scalar_first<float>(const float*, Layout, Halo<float>, const FieldsArgs&, ScalarGeom,
                                               ScalarRule, ScalarSource, ScalarUptake, ScalarEnds, ScalarGauges,
                                               const double*, double*, double*, hipStream_t);
template hipError_t launch_scalar_init<double>(const double*, Layout, Halo<double>, const FieldsArgs&, ScalarGeom,
                                               const double*, double*, hipStream_t);
template hipError_t launch_scalar_init<float>(const float*, Layout, Halo<float>, const FieldsArgs&, ScalarGeom,
                                              const double*, double*, hipStream_t);

}  // namespace iblb
