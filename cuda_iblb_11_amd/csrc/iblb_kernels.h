// iblb_kernels.h — host-callable launchers of the slab kernels (used by the ctx_*.hip files and iblb_ctx.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deep_plan.h"
#include "iblb_device.h"
#include "skip_box.h"

namespace iblb {

// Cells per lane of the collide-stream kernel: 16 bytes per lane per plane.
template <typename T>
constexpr int vec_of() { return 16 / (int)sizeof(T); }

// A slab's view of the points for IB with ghost columns (launch_ib_ghost below)
struct IbGhost {
    int nx, x_begin;
    int gc;        // ghost columns holding valid data (node pulls outside are skipped)
    int clo, chi;  // local columns that receive force
    int part;
    // the launch's first lane stores sig_val to *sig (agent scope) when the kernel starts: the kernels
    // before it in its stream are complete (the IB band cycle's exchange, ctx_band.hip)
    unsigned* sig = nullptr;
    unsigned sig_val = 0;
    // points [wlo, whi): their images -1 / +1 in groups of their own after the ns point groups (as
    // FusedArgs::wlo)
    int wlo = 0, whi = 0;
};

template <typename T>
struct FusedArgs {
    const T* src;
    T* dst;
    Layout L;
    Halo<T> H;          // column -1 / ncol planes (periodic images or ghost columns)
    int col_begin;      // first local column handled by this launch
    int col_step;       // distance between the columns of this launch (1 = contiguous range)
    int ncols;          // columns handled by this launch
    const int* cols;    // column table (device): column k of the launch is cols[col_begin + k]
                        // (nullptr: col_begin + k * col_step); IB bands of the K-iteration cycle
    int nch;            // 64*V-row chunks per column
    uint8_t* flags;     // per (column, chunk): dense IB force present (nullptr: no IB); the
                        // wave that consumes a chunk's force clears its values and its flag
                        // (columns -gc .. ncol+gc-1 addressable: the pointer is at column 0)
    double* fdense;     // dense IB force, x plane then y plane (column stride rows; column 0)
    long fplane;
    int flux_col;       // local column sampled for Q (>= 0), or -1 (none: never column -1, a ghost column)
    double flux_norm;
    double* Q;
    Coef c;
    KConst k;           // collide constants folded on the host (iblb_device.h)
    // IB band patches (band cycle, rows restricted): with row_tab set, cols holds 5 ints per entry
    // from col_begin on, {column, first chunk, end chunk, first row, end row}, and launch entry e
    // covers chunks [first, end) of its column (nchl waves per entry, the extra ones exit).  Q is
    // sampled on rows [first row, end row) only; store_rows: the populations too (other rows of
    // the column belong to the deep sweep).
    int row_tab = 0;
    int nchl = 0;
    int store_rows = 0;
    // Merged band chain (ctx_band.hip): the force of this level is read, not consumed (fkeep: the
    // IB waves below read it too); the waves of the entries clear the force buffer fdclr / flclr
    // of the level before (consumed by the previous launch) at their (column, chunk); clr_waves
    // more waves clear it at columns clr_lo .. clr_lo+clr_w-1 and clr_hi .. clr_hi+clr_w-1 (nch
    // chunks each); nns > 0: after those,
    // 16 lanes per point (nns points of the next level's iteration) evaluate the next level's force
    // from this launch's source (ib_next_group, ib_device.h) into fdnext / flnext.
    int fkeep = 0;
    double* fdclr = nullptr;
    uint8_t* flclr = nullptr;
    int clr_waves = 0, clr_lo = 0, clr_hi = 0, clr_w = 0;
    int nns = 0;
    IbGhost nG{};
    const float* n_s = nullptr;
    const float* n_us = nullptr;
    const int* n_eps = nullptr;
    double* fdnext = nullptr;
    uint8_t* flnext = nullptr;
    // points [wlo, whi): their periodic images (m = -1, +1) are evaluated by groups of their own after
    // the nns point groups, whose groups then take image m = 0 only (a point at the lattice's x edge
    // has two images in a slab touching that edge, which one group would walk one after the other)
    int wlo = 0, whi = 0;
    // vhalf (band cycle, f32): the launch's entry waves take 64 * V/2 rows (row_tab chunks in those
    // units); the IB flags stay per 64 * V rows, read at chunk / 2 and not cleared by these waves (two
    // waves share one: a flag left set over zeroed force takes the forced collide with force 0, bit
    // for bit the unforced one; a merged level's fdclr values are still cleared, their flag kept)
    int vhalf = 0;
};

// Two iterations per launch (lbm_sweep.hip): g^t -> g^{t+2}, no IB force owed in between.
// (SkipBox, MAX_SKIP: skip_box.h)

// (DeepBuild, the deep sweep's build features: deep_plan.h)

template <typename T>
struct Sweep2Args {
    const T* src;        // g^t
    T* dst;              // g^{t+K} (the other buffer)
    Layout L;
    int col_begin;       // sweep s covers output columns [col_begin + s*col_step, + W) ∩ [.., col_end)
    int col_step;
    int col_end;
    int nsweep;
    int W;               // output columns per sweep (wave)
    int vs;              // cells per lane; rows, col and plane multiples of vs
    int nch;             // set by launch_sweep2
    DeepBuild build;     // deep sweeps: the build's features
    int nsweep_w = 0;    // wall split (set by the launcher): sweeps of each wall chunk,
    int wall_ch0 = 0;    // inner chunks between the wall chunks,
    int wall_top = 0;    // and the first row of the top wall chunk
    int cus;             // deep sweeps, balanced widths: CUs the launch's stream may use (0 = all)
    int flux_col;        // local column sampled for Q (every iteration), or -1
    int fskip0, fskip1;  // rows [fskip0, fskip1) of the flux column are not sampled (an IB band
                         // patch covers them: its trapezoid's last level adds their flux)
    double flux_norm;
    double* Q;
    Coef c;
    KConst k;            // collide constants folded on the host (iblb_device.h)
    // Device-side ordering of a slab's interior and boundary sweeps (ghost-column builds only,
    // ctx_step.hip:deep_slab_step).  An edge wave is one whose output columns reach below wait_lo or
    // above wait_hi (wait_lo = INT_MAX: every wave).  wait_seq: edge waves first wait until
    // *wait_seq - wait_val >= 0, bounded by wait_ticks of the device's constant wall clock
    // (wall_clock64; the context's wait timeout, 600 s by default: a neighbour rank that is late
    // by less never fails the wait); past it they set *wait_err and go on, and the host reports the
    // call as failed.  done_cnt: edge waves add 1 when their stores are released (agent scope), and
    // the host learns their number from *edge_waves (set by the launcher).  nullptr: no wait / no signal.
    const unsigned* wait_seq = nullptr;
    unsigned wait_val = 0;
    int wait_lo = 0, wait_hi = 0;
    unsigned* wait_err = nullptr;
    unsigned long long wait_ticks = 0;
    unsigned* done_cnt = nullptr;
    int* edge_waves = nullptr;  // host pointer, written by launch_sweepk (not read on the device)
    int* kinfo = nullptr;       // host pointer: {MODE, VS, resident waves per SIMD, VGPRs, x-only force build} of the build launched
    int nskip = 0;       // > 0: the patch output regions below are left to the band's last level,
    SkipBox skip[MAX_SKIP];  // sorted by x0, disjoint in columns (a lone slab's deep sweep, a group slab's interior and boundary sweeps)
};

// ghost: false = lone slab (columns outside [0, ncol) are the periodic images; also the interior
// columns of a group slab, which read none); true = columns outside [0, ncol) are the ghost
// columns of the buffer itself (a group slab's boundary sweeps after the halo exchange)
template <typename T>
hipError_t launch_sweep2(Sweep2Args<T> a, bool ghost, hipStream_t s);
// K = depth (3 .. 7) iterations per launch: g^t -> g^{t+K}; ghost as above (a
// boundary sweep of output columns [0, K) reads columns -K .. 2K-1).  col_step 0: balanced widths.
// start / stop: recorded by the kernel's dispatch / completion signals (no marker packets)
template <typename T>
hipError_t launch_sweepk(Sweep2Args<T> a, int depth, bool ghost, hipStream_t s, hipEvent_t stop = nullptr,
                         hipEvent_t start = nullptr);
// *p = v after the stream's previous work (one lane, an agent-scope store: the release of the
// previous kernel's stores is its end-of-kernel fence)
hipError_t launch_seq_signal(unsigned* p, unsigned v, hipStream_t s);
// Test hold (IBLB_TEST_HOLD, ctx_step.hip:exchange): one wave that polls the host-coherent *word
// until it is non-zero or `ticks` of the device wall clock have passed, so that the work queued
// behind it on `s` starts late, as behind a neighbour rank that reaches its exchange late.
hipError_t launch_test_hold(const unsigned* word, unsigned long long ticks, hipStream_t s);
// Resident waves per CU of a deep-sweep configuration's plain build; *nch = its row chunks for ny rows.
template <typename T>
int sweepk_geometry(int depth, int vs, bool ghost, int ny, int* nch);

// Launch geometry of the collide-stream kernel: one wave per (column, 64*V-row chunk).
inline int chunks_per_column(int ny, int V) { return (ny + 64 * V - 1) / (64 * V); }

template <typename T>
hipError_t launch_fused(const FusedArgs<T>& a, hipStream_t s, hipEvent_t stop = nullptr);  // stop: recorded at the end

// Step 0 of a fresh state: collide f^0 with explicit rho^0, u^0, force^0 (no pull).
template <typename T>
hipError_t launch_boot(const T* src, T* dst, Layout L, const double* rho0, const double* u0,
                       const double* force0, long fplane, Coef c, KConst k, hipStream_t s);

// Macroscopic output in the reference layout (slab-local j = y*ncol + xc):
// rho = sum f, u = (sum c f + force/2)/rho with force = g + dense IB force.
template <typename T>
hipError_t launch_macro_out(const T* g, Layout L, Halo<T> H, const double* fdense, long fplane,
                            double gx, double gy, double* rho, double* u, hipStream_t s);

// Post-stream populations f^t in the reference AoS layout [9*j+i] (raw: no pull).
template <typename T>
hipError_t launch_pop_out(const T* g, Layout L, Halo<T> H, double* f, int raw, hipStream_t s);

// Windowed field readback (field_kernels.hip; include/iblb.h iblb_get_fields).  Sample (il, j) is the
// slab's cell (xl0 + il*sx, y0 + j*sy); plane k of out (the k-th set bit of `fields`) holds it at
// [(k*nyw + j)*nxl + il].
struct FieldsArgs {
    int xl0, sx, nxl;         // first sampled local column, stride, samples along x
    int y0, sy, nyw;          // first sampled row, stride, samples along y
    unsigned fields;          // IBLB_FIELD_* bits
    const double* fdense;     // dense IB force of the current state (nullptr: none)
    long fplane;
    double gx, gy;            // uniform body force
    const double* rho0;       // boot phase: rho^0 / u^0 (slab layout, plane stride fplane) instead of the
    const double* u0;         // moments, and the populations read in place (nullptr: run phase)
    double kvisc;             // -(1 - 1/(2 TAU)): stress = kvisc * PiNeq
    // the passive scalar's current populations (nullptr unless `fields` holds one of FIELD_SCALAR_BITS), five planes
    // sc[i * sc_plane + x * sc_rows + y] as ScalarGeom below
    const double* sc;
    long sc_rows, sc_plane;
};
// IBLB_FIELD_C | IBLB_FIELD_CUX | IBLB_FIELD_CUY: the fields that read the passive scalar.  Every reader kernel has
// a build with them and one without (a compile-time switch chosen at launch, like HEAVY).
constexpr unsigned FIELD_SCALAR_BITS = 4096u | 8192u | 16384u;
constexpr int FIELD_SCALAR_BIT0 = 12;  // the bit number of IBLB_FIELD_C; _CUX and _CUY follow
// Vorticity (IBLB_FIELD_VORT) wraps the neighbour columns modulo ncol: a lone slab only.
template <typename T>
hipError_t launch_fields_out(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, double* out, hipStream_t s);

// Window reduction (reduce_kernels.hip; include/iblb.h iblb_reduce_fields): statistics, row sums and
// column sums of the quantities in a.fields (the IBLB_FIELD_* and IBLB_QTY_* bits) over the samples of
// FieldsArgs, each evaluated once by the device functions of field_eval.h.
constexpr int REDUCE_NQ = 11;      // quantities of the fluid: bit k of `fields`, k < 11; bit 11 is none, and the
                                   // scalar's three (bits 12 .. 14) follow as quantities 11 .. 13 in the builds with them
constexpr int REDUCE_RS = 10;      // doubles of one statistics record: count, nonfinite, sum, sum_sq, min, max,
                                   // min_i, min_j, max_i, max_j (integers below 2^53: exact)
constexpr int REDUCE_ROWS = 256;   // window rows of one workgroup (one per lane, four waves)
// Pass 1 runs rb x cb workgroups: workgroup (r, c) takes window rows [256 r, 256 r + 256) and the slab's
// samples [cc c, cc c + cc) along x.  It leaves, each at its own fixed place in the scratch (doubles),
//   at 0      one statistics record per (workgroup, quantity)         [c * rb + r][nf][REDUCE_RS]
//   at o_row  one partial row sum per (column chunk, quantity, row)   [c][nf][nyw]        (rows)
//   at o_col  one partial column sum per (wave of rows, quantity, x)  [4 r + wave][nf][nxl] (cols)
// and pass 2, a launch of its own, adds them in ascending index order into the result at o_out:
// [nf][REDUCE_RS] records, then [nf][nyw] row sums (rows), then [nf][nxl] column sums (cols).
struct ReduceGeom {
    int cc, cb, rb;
    int nf;                    // quantities requested (set bits of a.fields)
    int i_first;               // window index i of the slab's first sample (min_i / max_i are window indices)
    int rows, cols;            // row sums / column sums wanted
    long o_row, o_col, o_out;  // offsets in the scratch
    long n_scratch, n_out;     // doubles of the whole scratch and of the result at its end
};
// The geometry for nxl x nyw samples (nxl, nyw >= 1): a function of the sizes and the request only.
ReduceGeom reduce_geometry(int nxl, int nyw, int nf, bool rows, bool cols);
// Both passes on stream s; the result is at scratch + q.o_out when they are done.  Vorticity as
// launch_fields_out: a lone slab only.
template <typename T>
hipError_t launch_reduce_fields(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, const ReduceGeom& q,
                                double* scratch, hipStream_t s);

// Point sampling and passive tracers (tracer_kernels.hip; include/iblb.h iblb_sample_points, iblb_set_tracers):
// one lane per point, its four cells evaluated by the device functions of field_eval.h.  Of FieldsArgs the
// window members are unused (fields, the force, the boot arrays and kvisc apply).  A lone slab only: the
// cells of a point wrap modulo ncol.
// out[k*n + p]: the k-th set bit of a.fields at the point (xy[p], xy[n + p]).
template <typename T>
hipError_t launch_sample_points(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, long n, const double* xy,
                                double* out, hipStream_t s);
// One explicit-Euler update of n tracers over `stride` iterations with the state held fixed.
template <typename T>
hipError_t launch_tracer_advect(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, long n, int stride, double* x,
                                double* y, int* laps, hipStream_t s);

// Tracers with a motion model (particle_kernels.hip; include/iblb.h iblb_set_tracer_model): the constants of one
// update.  amp = sqrt(6 D stride), m = the updates done before this one, t = the iteration of this one.
struct ParticleStep {
    double drift[2];
    double amp;
    int wall[2];
    unsigned long long seed;
    long long m, t;
};
// One update of the alive ones of n tracers over `stride` iterations with the state held fixed: the sample of
// launch_tracer_advect, the drift, a counter-based random step and the walls.  status and hit are written
// only where a tracer deposits.
template <typename T>
hipError_t launch_particle_advect(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, long n, int stride,
                                  const ParticleStep& P, double* x, double* y, int* laps, int* status, long long* hit,
                                  hipStream_t s);
// dep[floor(x[p])] += 1 for every tracer at the bottom, dep[ncol + floor(x[p])] += 1 for every one at the top;
// dep [2 ncol] is zeroed on the stream first.
hipError_t launch_particle_deposit(long n, int ncol, const double* x, const int* status, unsigned long long* dep,
                                   hipStream_t s);

// History recorder (history_kernels.hip; include/iblb.h iblb_set_history): one lane per probe, its four cells
// evaluated through point_eval.h exactly as launch_sample_points evaluates them.  The running statistics: eight
// arrays of np * n entries each, entry k*n + p for plane k of a record at probe p.
struct HistoryStats {
    long long* count;
    long long* nonfinite;
    double* sum;
    double* sum_sq;
    double* min;
    double* max;
    long long* min_rec;
    long long* max_rec;
};
// Record number m of n probes at (x[p], y[p]) into slot[k*n + p] and into the statistics, plane k the k-th set bit
// of a.fields.  laps != nullptr: the probes are tracers, the record starts with the planes x, y, (double)laps and
// a.fields may be 0.  A lone slab only, as launch_sample_points.
template <typename T>
hipError_t launch_history_record(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, long n, const double* x,
                                 const double* y, const int* laps, long long m, double* slot, const HistoryStats& s,
                                 hipStream_t st);

// Time- and phase-averaged fields (average_kernels.hip; include/iblb.h iblb_set_average).  One bin's
// accumulators are `planes` planes of nxl * nyw doubles in the order the lanes run, [plane][il*nyw + j]:
// the sums of the set bits of a.fields in ascending order, then their sums of squares (IBLB_AVG_SQ),
// then one plane of ux*uy (IBLB_AVG_UXUY).
// Adds the samples of FieldsArgs, each evaluated once by the device functions of field_eval.h, into the
// bin at acc.  Vorticity as launch_fields_out: a lone slab only.
template <typename T>
hipError_t launch_average_accum(const T* g, Layout L, Halo<T> H, const FieldsArgs& a, unsigned flags, double* acc,
                                hipStream_t s);
// The planes of one bin transposed into iblb_get_fields' layout: out[(p*nyw + j)*nxl + il].
hipError_t launch_average_readout(const double* acc, int nxl, int nyw, int planes, double* out, hipStream_t s);

// Passive scalar (scalar_kernels.hip; include/iblb.h iblb_set_scalar): a D2Q5 lattice of five planes of doubles,
// s[i * plane + x * rows + y], two such buffers and a two-plane velocity scratch uv in the same order.
struct ScalarGeom {
    int ncol, ny;
    long rows;   // column stride (Layout::rows)
    long plane;  // plane stride: ncol * rows
};
struct ScalarRule {
    double omega;          // 1.0 / tau
    int wall_kind[2];      // IBLB_SCALAR_WALL_*: below row 0, above row ny - 1
    double wall_value[2];
};
// The scalar's source (include/iblb.h iblb_set_scalar_source).  field == nullptr: none, and every launch below runs
// the build without it.  Otherwise all three members are set: a NULL array of the ABI is a device array of zeros
// (wall_value: of the uniform value), so that the kernels have no per-pointer branch.
struct ScalarSource {
    const double* field;  // one plane [x * rows + y]: s(x, y)
    const double* walls;  // [4 * ncol]: wall_flux[0], wall_flux[1], wall_value[0], wall_value[1], [ncol] each
    double decay;
};
// The scalar's uptake (include/iblb.h iblb_set_scalar_uptake).  a == nullptr: none, and every launch below runs the
// build without it.  Otherwise all three members are set, [2 * ncol] each, index k * ncol + x for wall k (0: below
// row 0, 1: above row ny - 1): a NULL rate array of the ABI is held as zeros in `a`.
struct ScalarUptake {
    const double* a;  // a_k[x] = 2.0 - 2.0/(1.0 + 3.0*rate[k][x]), computed on the host
    double* total;    // what crossed wall k of column x since the set / the reset
    double* last;     // ... during the last substep
};
// The scalar's open ends in x (include/iblb.h iblb_set_scalar_ends).  value == nullptr: none (the scalar is periodic
// in x), and every launch below runs the build without them.  Otherwise all three arrays are set, [2 * ny] each, index
// k * ny + y for end k (0: left of column 0, 1: right of column ncol - 1): a NULL profile of the ABI is held as an
// array of the uniform value, so that the kernels have no per-pointer branch.
struct ScalarEnds {
    int kind[2];          // IBLB_SCALAR_END_*
    const double* value;  // the value of row y at a _VALUE end
    double* total;        // what crossed end k in row y since the set / the reset
    double* last;         // ... during the last substep
};
// The scalar's transport gauges (include/iblb.h iblb_set_scalar_gauges).  col == nullptr: none, and every launch below
// runs the build without them.  Otherwise all six members are set.  col[x] = {the station whose column is x, the
// station whose column is x's left neighbour (ncol - 1 for x == 0)} and row[y] = {the level whose row is y, the level
// whose row is y - 1}, -1 where there is none: the first is the entry whose right / up the lane of cell (x, y) adds
// to, the second the one whose left / down it adds to.  A count of 0 leaves its pair of totals empty and its indices -1.
struct ScalarGauges {
    const int2* col;  // [ncol]
    const int2* row;  // [ny]
    double* right;    // [n_stations * ny], index k * ny + y: sum of p_1(station[k], y)
    double* left;     // ... of p_2(station[k] + 1, y)
    double* up;       // [n_levels * ncol], index k * ncol + x: sum of p_3(x, level[k])
    double* down;     // ... of p_4(x, level[k] + 1)
};
// One substep src -> dst (distinct buffers).  first: the velocity from the fluid state by cell_state of
// field_eval.h (of FieldsArgs the window members are unused), also left in uv; next: the velocity read from uv.
// With an uptake the lanes of rows 0 and ny - 1 also update U.total and U.last, one writer per entry; with open ends
// the lanes of columns 0 and ncol - 1 likewise E.total and E.last; with gauges the lanes beside a gauged link G's
// four totals.
template <typename T>
hipError_t launch_scalar_first(const T* f, Layout L, Halo<T> H, const FieldsArgs& a, ScalarGeom S, ScalarRule R,
                               ScalarSource Q, ScalarUptake U, ScalarEnds E, ScalarGauges G, const double* src,
                               double* dst, double* uv, hipStream_t s);
hipError_t launch_scalar_next(ScalarGeom S, ScalarRule R, ScalarSource Q, ScalarUptake U, ScalarEnds E, ScalarGauges G,
                              const double* src, double* dst, const double* uv, hipStream_t s);
// dst's five planes = the equilibrium of C = c[x * rows + y] at the fluid state's velocity; c may be dst's plane 0.
template <typename T>
hipError_t launch_scalar_init(const T* f, Layout L, Halo<T> H, const FieldsArgs& a, ScalarGeom S, const double* c,
                              double* dst, hipStream_t s);
// `planes` (1 .. 5) planes in the reference layout, ref[p * ncol * ny + y * ncol + x], into dev's planes; the five
// planes of dev out the same way; C = (((g0+g1)+g2)+g3)+g4 on a window (validated by the caller) into
// out[j * nxw + i].
hipError_t launch_scalar_in(const double* ref, ScalarGeom S, int planes, double* dev, hipStream_t s);
hipError_t launch_scalar_populations_out(const double* dev, ScalarGeom S, double* out, hipStream_t s);
hipError_t launch_scalar_out(const double* dev, ScalarGeom S, int x0, int y0, int nxw, int nyw, int sx, int sy,
                             double* out, hipStream_t s);
// The wall flux of the last substep (include/iblb.h iblb_get_scalar_wall_flux): out[x] through the wall below row 0,
// out[ncol + x] through the wall above row ny - 1.  With a source: its wall_flux at a no-flux wall, its wall_value
// in the expression of a _VALUE wall.
hipError_t launch_scalar_wall_flux(const double* dev, ScalarGeom S, ScalarRule R, ScalarSource Q, double* out,
                                   hipStream_t s);
// One plane out in the reference layout: out[y * ncol + x] = dev[x * rows + y] (iblb_get_scalar_source).
hipError_t launch_scalar_plane_out(const double* dev, ScalarGeom S, double* out, hipStream_t s);

// q(u^t) of the current state for the flux column (added to *out).
template <typename T>
hipError_t launch_flux(const T* g, Layout L, Halo<T> H, const double* fdense, long fplane,
                       double gx, double gy, int xc, double flux_norm, double* out, hipStream_t s);

// Non-finite stored populations of the slab's own cells (rows < ny, all nine planes), added to
// *count (one double: an exact integer up to 2^53).
template <typename T>
hipError_t launch_count_nonfinite(const T* g, Layout L, double* count, hipStream_t s);

// Reference AoS populations [9*j+i] -> slab planes (deviation form for float).
template <typename T>
hipError_t launch_pop_in(const double* f, T* g, Layout L, hipStream_t s);

// Reference SoA field [comp*N + j] (j = y*ncol + xc) <-> slab layout [comp*fplane + xc*col + y].
hipError_t launch_field_in(const double* ref, double* lay, Layout L, int ncomp, long fplane, hipStream_t s);
hipError_t launch_field_out(const double* lay, double* ref, Layout L, int ncomp, long fplane, double add0,
                            double add1, hipStream_t s);

// Immersed boundary (global coordinates; the slab owns columns [x_begin, x_begin+ncol)).
// Single slab: nodes + interpolation + spread of every point in one launch.
template <typename T>
hipError_t launch_ib_point(const T* g, Layout L, Halo<T> H, int nx, int ns, const float* s, const float* u_s,
                           const int* eps, float* F_s, double* fdense, long fplane, uint8_t* flags, int nch,
                           int rows_per_chunk, hipStream_t st);
// A slab with ghost columns (a slab of a group after a halo exchange of depth >= gc, or a lone
// slab whose ghosts hold periodic copies): every point whose 3x3 spread reaches local columns
// [clo, chi) — each periodic image of it, x0 - x_begin + m * nx for m = -1, 0, 1 — pulls its nodes
// from the buffer (columns -gc .. ncol+gc-1) and spreads into the cells of [clo, chi) (global
// columns clipped to [0, XDIM) as the reference's cell-centric spread).  F_s: the slab holding
// column min(x0, XDIM-1) writes the point's F_s, the others zero (readers sum).  part: 0 every
// point, 1 the inner points (2 <= x0 - x_begin <= ncol-3: nodes and pulls inside the slab, no
// ghost needed), 2 the others.
// (IbGhost: declared with FusedArgs above)
template <typename T>
hipError_t launch_ib_ghost(const T* g, Layout L, IbGhost G, int ns, const float* s, const float* u_s, const int* eps,
                           float* F_s, double* fdense, long fplane, uint8_t* flags, int nch, int rows_per_chunk,
                           hipStream_t st);

}  // namespace iblb
