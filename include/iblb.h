/*
 * iblb.h — C ABI of the MI355X-native immersed-boundary lattice-Boltzmann hot path.
 *
 * Replaces the hot path of ptheywood/CUDA_IBLB_11 (reference @ /root/reference):
 *   LatticeBoltzmann.cuh:4-10  equilibrium / collision / streaming / macro kernels
 *   ImmersedBoundary.cuh:4-8   interpolate / spread kernels
 *   main.cu:817-934            the per-step launch sequence that drives them
 *
 * Two layers are exported:
 *
 *  (1) Reference-shaped entry points (iblb_equilibrium ... iblb_spread).  Same names,
 *      same argument lists and the same array layouts as the reference kernels
 *      (device pointers; f/f0/f1/F are AoS [9*j+i], u/force are SoA [a*size+j],
 *      Lagrangian arrays are interleaved float xy), plus a trailing HIP stream.
 *      A maintainer replaces `kernel<<<grid, block, 0, s>>>(args)` in main.cu by
 *      `iblb_kernel(args, s)`.  They keep the reference's unfused data flow and exist
 *      for drop-in compatibility and kernel-by-kernel parity, not for speed.
 *
 *  (2) The fused context API (iblb_create ... iblb_destroy).  One context owns one
 *      x-slab of the lattice on one GPU, stores the populations SoA (y fastest) and
 *      advances the exact reference time step
 *        equilibrium -> collision -> streaming -> macro -> interpolate -> spread
 *      (main.cu:852-909): without IB one bandwidth-bound kernel advances up to seven
 *      iterations (temporal blocking, the deep sweep), with IB a band cycle of K iterations
 *      (the deep sweep beside a chain of small launches around the points).  Host arrays crossing this boundary use the reference layouts
 *      restricted to the slab: cell j = y * x_count + (x - x_begin).
 *
 * Conventions: every function returns IBLB_OK (0) or a negative IBLB_ERR_* code;
 * no C++ exception crosses the ABI.  The caller owns host buffers, the library owns
 * device buffers.  One host thread per context.  Context calls are synchronous on
 * return (results are in the caller's buffers).  The reference had no error
 * channel other than cudaGetLastError() at the call sites (main.cu:724-728,
 * 854-887, 902-922); here the code is returned and iblb_last_error() explains it.
 */
#ifndef IBLB_H
#define IBLB_H

#ifdef __cplusplus
extern "C" {
#endif

#define IBLB_OK               0
#define IBLB_ERR_ARG         -1   /* invalid argument / shape                      */
#define IBLB_ERR_HIP         -2   /* HIP runtime error (message in last_error)     */
#define IBLB_ERR_STATE       -3   /* call not valid in the current context state   */
#define IBLB_ERR_COMM        -4   /* RCCL / transport error                        */
#define IBLB_ERR_NOMEM       -5   /* device or host allocation failed              */
#define IBLB_ERR_UNSUPPORTED -6   /* feature not built / not available             */
#define IBLB_ERR_NODEVICE    -7   /* no HIP device visible                         */

#define IBLB_PREC_F64 0          /* populations stored and collided in double      */
#define IBLB_PREC_F32 1          /* populations stored as float deviations f - w_i */

#define IBLB_UNIQUE_ID_BYTES 128 /* size of the RCCL unique id blob               */

/* ABI version of this header: bumped whenever a struct crossing the ABI changes layout (iblb_config,
 * iblb_timing, iblb_cilia).  5: iblb_timing's band_cycles ... deep_iterations (round 4), the
 * size-checked iblb_get_timing_ex (round 5).  6: iblb_timing's dev_wait_launches and deep_mode ... deep_vgprs, and
 * iblb_set_wait_timeout (round 6).  Compare with iblb_abi_version() at run time. */
#define IBLB_ABI_VERSION 6

/* ---------------------------------------------------------------------------------
 * (1) Reference-shaped kernels.  All pointers are DEVICE pointers.  `stream` is a
 * hipStream_t (NULL = default stream).  Launch is asynchronous, like the reference's
 * <<< >>> launches; the return value reports launch errors only.
 * ------------------------------------------------------------------------------- */

/* LatticeBoltzmann.cu:30 equilibrium(u, rho, f0, force, F, XDIM, YDIM, TAU) */
int iblb_equilibrium(const double* u, const double* rho, double* f0, const double* force,
                     double* F, int XDIM, int YDIM, double TAU, void* stream);

/* LatticeBoltzmann.cu:64 collision(f0, f, f1, F, TAU, TAU2, XDIM, YDIM, it) — `it` unused as in the reference */
int iblb_collision(const double* f0, const double* f, double* f1, const double* F,
                   double TAU, double TAU2, int XDIM, int YDIM, int it, void* stream);

/* LatticeBoltzmann.cu:173 streaming(f1, f, XDIM, YDIM) */
int iblb_streaming(const double* f1, double* f, int XDIM, int YDIM, void* stream);

/* LatticeBoltzmann.cu:375 macro(f, u, rho, XDIM, YDIM) */
int iblb_macro(const double* f, double* u, double* rho, int XDIM, int YDIM, void* stream);

/* ImmersedBoundary.cu:94 interpolate(rho, u, Ns, u_s, F_s, s, XDIM, YDIM) */
int iblb_interpolate(const double* rho, const double* u, int Ns, const float* u_s, float* F_s,
                     const float* s, int XDIM, int YDIM, void* stream);

/* ImmersedBoundary.cu:138 spread(rho, u, f, Ns, u_s, F_s, force, s, XDIM, Q, epsilon).
 * Like the reference it assumes YDIM == 192 (`size = 192 * XDIM`, ImmersedBoundary.cu:146)
 * and accumulates Q += u_x(XDIM-5, y)/192 (ImmersedBoundary.cu:259-264). */
int iblb_spread(const double* rho, double* u, const double* f, int Ns, const float* u_s,
                const float* F_s, double* force, const float* s, int XDIM, double* Q,
                const int* epsilon, void* stream);

/* spread with the grid height, flux column and flux divisor made explicit
 * (YDIM == 192, flux_column == XDIM-5, flux_norm == 192 reproduces iblb_spread). */
int iblb_spread_ex(const double* rho, double* u, const double* f, int Ns, const float* u_s,
                   const float* F_s, double* force, const float* s, int XDIM, int YDIM,
                   double* Q, const int* epsilon, int flux_column, double flux_norm,
                   void* stream);

/* ImmersedBoundary.cu:21 d_delta, evaluated on the device for n (xs, ys, x, y) tuples
 * (parity hook for the 3-point kernel). */
int iblb_delta(int n, const float* xs, const float* ys, const int* x, const int* y,
               float* out, void* stream);

/* main.cu:77 define_filament(T, it, c_space, p_step, c_num, s, lasts, b_points): cilia beat
 * shape, s = the reference's d_boundary [5*9600*c_num], lasts [2*9600*c_num], b_points
 * [5*96*c_num].  Where two samples qualify for one boundary point the later one in thread
 * order is kept (the reference leaves that race unspecified). */
int iblb_define_filament(int T, int it, double c_space, int p_step, double c_num, float* s,
                         float* lasts, float* b_points, void* stream);

/* main.cu:176 boundary_check(c_space, c_num, XDIM, it, b_points, s, u_s, epsilon): Lagrangian
 * points s [2*96*c_num], velocities u_s and overlap mask epsilon [96*c_num]. */
int iblb_boundary_check(double c_space, int c_num, int XDIM, int it, const float* b_points,
                        float* s, float* u_s, int* epsilon, void* stream);

/* ---------------------------------------------------------------------------------
 * (2) Fused context API.
 * ------------------------------------------------------------------------------- */

typedef struct iblb_ctx iblb_ctx;

typedef struct iblb_config {
    int    nx, ny;            /* global lattice XDIM x YDIM (main.cu:270-271,298)          */
    double tau, tau2;         /* TAU, TAU2 (main.cu:320-321)                               */
    int    precision;         /* IBLB_PREC_F64 (default) or IBLB_PREC_F32                  */
    double body_force[2];     /* uniform force added to force^t every step; (0,0) = ref.  */
    double flux_norm;         /* Q += u_x / flux_norm; reference literal 192 (IB.cu:261)   */
    int    flux_column;       /* global column sampled for Q; reference XDIM-5 (IB.cu:259) */
    int    device;            /* HIP device ordinal                                        */
    int    x_begin, x_count;  /* owned columns [x_begin, x_begin + x_count); x_count <= 0
                                 means the whole lattice (single slab)                     */
    int    max_points;        /* Lagrangian point capacity; 0 disables the IB kernels      */
} iblb_config;

typedef struct iblb_timing {
    long long steps;           /* reference steps completed                              */
    long long fused_launches;  /* collide-stream launches timed                          */
    double    fused_ms;        /* summed duration of the timed collide-stream launches   */
    double    ib_ms;           /* summed duration of IB phases (interp + spread)         */
    double    halo_ms;         /* summed duration of halo exchanges                      */
    double    fused_bytes;     /* algorithmic bytes per cell of the collide-stream kernel */
    long long cells;           /* cells owned by this context                            */
    long long fused_cells;     /* lattice updates done by the timed collide-stream launches */
    /* two-iteration launches (temporal blocking, lbm_sweep.hip): each reads and writes the
     * state once (fused_bytes per cell) and advances its cells by two iterations */
    long long sweep_launches;  /* timed two-iteration launches                           */
    double    sweep_ms;        /* their summed duration                                  */
    long long sweep_cells;     /* cells they covered (lattice updates = 2 x sweep_cells) */
    /* deep launches (IBLB_SWEEP_DEPTH = K >= 3): state read and written once for K (or K-1)
     * iterations */
    long long sweepk_launches;
    double    sweepk_ms;
    long long sweepk_cells;    /* cells they covered; lattice updates = sweepk_cells x the launches'
                                * depths (deep_iterations / deep_launches on average) */
    long long sweepk_depth;    /* K, the configured depth */
    /* IB band cycles run (ctx_band.hip), and how many of them ran the merged chain; counted
     * whether or not profiling events are on */
    long long band_cycles;
    long long band_merged_cycles;
    long long band_par_cycles;  /* of those, run with the last level beside the deep sweep (lone slab) */
    /* deep launches (lone slab, slab interiors, band cycles) and the iterations they advanced, counted
     * whether or not profiling events are on: a call of n iterations mixes depths K and K-1 so that
     * no two-iteration or one-step remainder is left where n allows it (deep_plan.h:deep_depth) */
    long long deep_launches;
    long long deep_iterations;
    /* launches of an RCCL group slab whose waves waited on a device word instead of a queue wait
     * (the slab hand-off, iblb_set_wait_timeout below); counted without profiling */
    long long dev_wait_launches;
    /* the build of the last deep launch (lone slab, slab interior or band cycle's deep sweep): its
     * MODE bits (lbm_sweep_impl.h), cells per lane, resident waves per SIMD and VGPRs per lane */
    long long deep_mode, deep_vs, deep_waves_per_simd, deep_vgprs;
} iblb_timing;

/* Reference defaults: 288x192, TAU/TAU2 for Re=1, T=1e5 (main.cu:267-321). */
int iblb_config_default(iblb_config* cfg);

int  iblb_create(const iblb_config* cfg, iblb_ctx** out);
void iblb_destroy(iblb_ctx* ctx);
const char* iblb_last_error(const iblb_ctx* ctx);   /* NULL ctx: last create() error */
const char* iblb_version(void);
int  iblb_abi_version(void);                       /* IBLB_ABI_VERSION the library was built with */
int  iblb_device_count(int* n);

/* Initial state (main.cu:636-754).  rho [N], u [2N] SoA, force [2N] SoA (force^0, may be
 * NULL = 0), f [9N] AoS post-stream populations (NULL = feq(rho, u) exactly as the
 * reference's initial `equilibrium` launch, main.cu:722-754).  N = x_count * ny.
 * rho == NULL and u == NULL: rho = 1, u = 0 (the reference's initial values). */
int iblb_set_state(iblb_ctx* ctx, const double* rho, const double* u, const double* f,
                   const double* force);

/* Lagrangian points for the next immersed-boundary evaluation (main.cu:834 boundary_check
 * outputs): s [2ns] xy, u_s [2ns] xy, epsilon [ns] (NULL = all 1).  Global coordinates.
 * A slab of a group needs >= 3 columns and the reference's invariant 0 <= s_x <= XDIM
 * (boundary_check wraps s_x into it, main.cu:202-205); IBLB_ERR_ARG otherwise.
 * Points replaced in mid-run still owe their force to the next iteration: it is evaluated
 * before the new points are taken, and the next iblb_step starts with a one-step iteration
 * that applies it (then band cycles again). */
int iblb_set_lagrangian(iblb_ctx* ctx, int ns, const float* s, const float* u_s,
                        const int* epsilon);

/* Lagrangian points of the next `nsteps` iterations, given ahead (the reference computes a
 * new s, u_s, epsilon every iteration before its IB step, main.cu:822-841, 900-909): iteration
 * t0 + i (t0 = iblb_get_step at the call) uses entry i; after the last entry the points stay
 * those of entry nsteps-1.  Same result as iblb_set_lagrangian(entry i) before each of those
 * iterations, but iblb_step can then advance several iterations per launch (IB band cycle)
 * where the points of one cycle force only part of the lattice.  s, u_s [nsteps][2ns] xy,
 * epsilon [nsteps][ns] (NULL = all 1).  iblb_set_lagrangian / iblb_set_cilia end the schedule.
 * iblb_set_state keeps a schedule and re-bases it: iteration i of the new state uses entry i
 * (clamped to the last).  Until the first step iblb_get_lagrangian returns the points that were
 * current before the call. */
int iblb_set_lagrangian_steps(iblb_ctx* ctx, int nsteps, int ns, const float* s, const float* u_s,
                              const int* epsilon);

/* On-device cilia kinematics (main.cu:822-841): when set, every iblb_step iteration `it`
 * first runs define_filament + boundary_check for `it` and uses their s, u_s, epsilon as the
 * Lagrangian points of that iteration (no host round trip).  c_num <= 0 or NULL disables.
 * Needs max_points >= 96 * c_num.  Excludes iblb_set_lagrangian while active.
 * The kinematics start at the context's current iteration with zeroed history (the reference's
 * `lasts`), and u_s is the displacement since the previous iteration: that gives a meaningful
 * u_s only from iteration 0 (u_s(0) = 0 exactly), so set the cilia before the state, or at
 * iteration 0.  A fresh start at it = 7 gives |u_s| of about 234 lattice units per iteration
 * for that one iteration.  iblb_set_state restarts the beat (history zeroed, it = 0);
 * a checkpoint holds the configuration and the history. */
typedef struct iblb_cilia {
    int    c_num;    /* cilia (main.cu:268)                                        */
    double c_space;  /* spacing of the cilium bases in lattice units (main.cu:280) */
    int    T;        /* beat period in iterations (main.cu:299)                    */
    int    p_step;   /* phase lag of neighbouring cilia, T*c_fraction/c_num (main.cu:336) */
} iblb_cilia;
int iblb_set_cilia(iblb_ctx* ctx, const iblb_cilia* cilia);
/* Current Lagrangian points (the reference's d_s, d_u_s, d_epsilon; any may be NULL). */
int iblb_get_lagrangian(iblb_ctx* ctx, float* s, float* u_s, int* epsilon);

/* Advance nsteps reference iterations (main.cu:852-909 each). */
int iblb_step(iblb_ctx* ctx, int nsteps);

/* Macroscopic fields after the last step as the reference holds them after `spread`:
 * rho [N] = sum f (macro), u [2N] SoA = (sum c f + force/2)/rho.  Either may be NULL. */
int iblb_get_macro(iblb_ctx* ctx, double* rho, double* u);
/* Post-stream populations f^t [9N] AoS (the reference's d_f after streaming). */
int iblb_get_populations(iblb_ctx* ctx, double* f);
/* force^t [2N] SoA as the reference's d_force after spread (plus body_force). */
int iblb_get_force(iblb_ctx* ctx, double* force);
/* Lagrangian force F_s [2ns] of the last interpolation.  Collective in an RCCL group; in a
 * local group each slab holds the F_s of the points whose column min(x0, XDIM-1) it owns and
 * zeros for the others (sum over the slabs). */
int iblb_get_lagrangian_force(iblb_ctx* ctx, float* F_s);
/* Cumulative flux Q (ImmersedBoundary.cu:259-264).  With a multi-slab RCCL group this
 * is the sum over all ranks; with a local group it is this slab's share. */
int iblb_get_flux(iblb_ctx* ctx, double* Q);
int iblb_get_step(iblb_ctx* ctx, long long* steps);
/* Non-finite (NaN / Inf) stored populations of the current state, counted over every cell
 * of the lattice (summed over the ranks of an RCCL group: collective).  The driver checks it
 * at every output iteration (the reference's penalty IB can diverge). */
int iblb_count_nonfinite(iblb_ctx* ctx, long long* count);

/* Windowed field readback: chosen fields on a strided window of the lattice, computed on the device
 * and copied out at the window's size (not the lattice's).  The window samples the global cells
 * (x0 + i*sx, y0 + j*sy), i < nx, j < ny: sx, sy >= 1, nx, ny >= 1, every sampled cell inside
 * [0, XDIM) x [0, YDIM); the window never wraps.  NULL means the whole lattice at stride 1. */
typedef struct iblb_window { int x0, y0, nx, ny, sx, sy; } iblb_window;   /* global cells x0+i*sx, y0+j*sy */
#define IBLB_FIELD_RHO 1   /* as iblb_get_macro */
#define IBLB_FIELD_UX  2
#define IBLB_FIELD_UY  4
#define IBLB_FIELD_VORT 8  /* d(uy)/dx - d(ux)/dy */
#define IBLB_FIELD_SXX 16  /* viscous stress -(1 - 1/(2 TAU)) * PiNeq_ab */
#define IBLB_FIELD_SXY 32
#define IBLB_FIELD_SYY 64
/* The passive scalar (iblb_set_scalar below) through the same readers; bits 128 .. 1024 are iblb_reduce_fields'
 * own quantities and 2048 is no bit.  Each is defined bit-exactly, in double, one rounding per operation, no
 * contraction:
 *   C   = (((g0+g1)+g2)+g3)+g4 of the scalar's stored populations at the moment of the call: what iblb_get_scalar
 *         returns for that cell, bit for bit.  Between two events of the scalar it is the C of the last event,
 *         while ux, uy are those of the current state.
 *   CUX = C*ux, CUY = C*uy with ux, uy the IBLB_FIELD_UX / _UY values of that cell at that moment.
 * Accepted by iblb_get_fields, iblb_reduce_fields, iblb_sample_points (the product is formed per cell, then
 * interpolated) and iblb_set_average (which adds v, and v*v under IBLB_AVG_SQ, as for any field: <ux C> is the
 * sum plane of IBLB_FIELD_CUX), ordered with the other bits by ascending bit, in every phase.  With no scalar
 * set, and always on a slab of a local or RCCL group (which cannot hold one), a request with one of these bits
 * returns IBLB_ERR_STATE: checked after the argument checks and the vorticity check below, before anything
 * collective or any launch, no output touched. */
#define IBLB_FIELD_C   4096   /* the passive scalar, as iblb_get_scalar returns it for that cell */
#define IBLB_FIELD_CUX 8192   /* C*ux : advective flux density, one rounding */
#define IBLB_FIELD_CUY 16384  /* C*uy */
/* The samples of window w whose column this context owns: sample indices [*i_first, *i_first +
 * *nx_local) of the window's nx (nx_local may be 0; either pointer may be NULL). */
int iblb_window_local(iblb_ctx* ctx, const iblb_window* w, int* i_first, int* nx_local);
/* For the k-th set bit of `fields` in ascending bit order, out[(k*ny + j)*nx_local + il] is that field
 * at sample (i_first + il, j).  nx_local == 0: IBLB_OK, nothing written.  fields == 0, an unknown bit, a
 * bad window, or out == NULL with nx_local > 0: IBLB_ERR_ARG (checked before anything collective).
 * Valid in every phase, before the first step included.  Every field is a function of exactly what
 * iblb_get_macro (rho, u with the force/2 correction) and iblb_get_populations (f) return at that moment:
 *   PiNeq_ab = sum_i c_ia c_ib (f_i - feq_i(rho, u)), feq the reference equilibrium
 *   (LatticeBoltzmann.cu:45-49, C_S = 0.57735) evaluated in double; the O(u F) term that Guo forcing
 *   adds to the second moment is left out of the stress.
 *   Vorticity: central differences of u at lattice spacing 1 whatever the stride, periodic in x; at
 *   y = 0 and y = YDIM-1 the one-sided first difference.
 * Vorticity needs the neighbour columns' u and force: a lone slab computes it; a slab of a local or
 * RCCL group returns IBLB_ERR_UNSUPPORTED when IBLB_FIELD_VORT is set (every other field works).
 * Goes through the same preparation as every reader: collective in an RCCL group, where each rank
 * receives its own samples. */
int iblb_get_fields(iblb_ctx* ctx, const iblb_window* w, unsigned fields, double* out);

/* Window reduction: statistics, row sums and column sums of chosen quantities over a window, computed on
 * the device; what crosses to the host is O(nx + ny) values, not the window.  `w`, the IBLB_FIELD_* bits (the
 * scalar's three included) and the value of every sample are exactly those of iblb_get_fields (every phase, the boot phase
 * included); four more quantities are accepted here only (iblb_get_fields refuses them), each the stated
 * expression of that sample's rho, ux, uy with one rounding per operation: */
#define IBLB_QTY_MOMX 128    /* rho*ux */
#define IBLB_QTY_MOMY 256    /* rho*uy */
#define IBLB_QTY_KE   512    /* 0.5*(rho*(ux*ux + uy*uy)), evaluated in exactly this order */
#define IBLB_QTY_USQ  1024   /* ux*ux + uy*uy  (Ma^2 = max / C_S^2; no sqrt on the device) */
typedef struct iblb_field_stats {
    long long count;       /* finite samples reduced */
    long long nonfinite;   /* NaN / Inf samples: counted here and left out of everything else */
    double sum, sum_sq;
    double min, max;       /* count == 0: +inf / -inf */
    int min_i, min_j, max_i, max_j;  /* window sample indices (i of the window's nx, not slab-local); count == 0: -1 */
} iblb_field_stats;
/* stats[k] (and row k of row_sum, col_sum) belongs to the k-th set bit of `fields` in ascending bit order.
 * This context reduces the samples whose column it owns (iblb_window_local): row_sum[k*w.ny + j] is the
 * sum over its i of row j, col_sum[k*nx_local + il] the sum over j of its sample column il; either may be
 * NULL (not computed).  min / max compare with < / >; among equal values the sample with the lowest j,
 * then the lowest i, is reported (the first in row-major order).  A non-finite sample of a quantity is
 * counted in `nonfinite` and is absent from that quantity's count, sums, extrema, row and column sums.
 * nx_local == 0: IBLB_OK, empty statistics (count 0, +inf / -inf, -1), row_sum zeros, col_sum untouched.
 * The result is a function of the state and the window alone (no floating-point atomics; fixed summation
 * order): repeated calls return the same bits.  sum and sum_sq are within n * 2^-53 * sum |x| (sum x^2) of
 * the exact sum of the n samples.
 * fields == 0, an unknown bit, a bad window or stats == NULL: IBLB_ERR_ARG, checked before anything
 * collective, no output touched.  IBLB_FIELD_VORT on a slab of a local or RCCL group: IBLB_ERR_UNSUPPORTED
 * (as iblb_get_fields).  Collective in an RCCL group like every reader; each rank receives its own part
 * (combining the parts is the caller's: counts and sums add, extrema follow the tie rule, row sums add,
 * column sums concatenate in slab order). */
int iblb_reduce_fields(iblb_ctx* ctx, const iblb_window* w, unsigned fields, iblb_field_stats* stats,
                       double* row_sum, double* col_sum);

/* Point sampling: chosen fields at n arbitrary points, interpolated on the device; the points cross in one
 * copy and the results return in one.  x, y [n] are host arrays in global lattice coordinates, `fields` the
 * IBLB_FIELD_* bits of iblb_get_fields, out[k*n + p] the k-th set bit (ascending) at point p.  A point needs 0 <= x < XDIM
 * and 0 <= y <= YDIM-1, both finite.  With
 *   i0 = floor(x), i1 = (i0 + 1) mod XDIM (periodic), a = x - i0,
 *   j0 = min(floor(y), YDIM-2), j1 = j0 + 1, b = y - j0  (y = YDIM-1: b = 1 on the top row)
 * and vIJ the value iblb_get_fields returns for cell (iI, jJ) at that moment, bit for bit,
 *   v = (1-b)*((1-a)*v00 + a*v10) + b*((1-a)*v01 + a*v11)
 * in double, one rounding per operation, no contraction.  Valid in every phase, the boot phase included.
 * n < 0, a NULL pointer with n > 0, fields == 0, an unknown bit, YDIM < 2, or any point out of range or
 * non-finite: IBLB_ERR_ARG, checked before any launch, no output touched.  n == 0: IBLB_OK.  A slab of a
 * local or RCCL group: IBLB_ERR_UNSUPPORTED (a point's four cells may straddle slabs). */
int iblb_sample_points(iblb_ctx* ctx, int n, const double* x, const double* y, unsigned fields, double* out);

/* Passive tracers: n points the context itself moves with the fluid while iblb_step runs, so that following
 * fluid parcels needs no readback and keeps the deep sweep between their updates.  On the device they are
 * x[n], y[n] in double and laps[n] in int.  The positions must be double: at x ~ 4096 a float's ulp is 4.9e-4,
 * more than one iteration's displacement at this project's Mach numbers, so a float position would not move.
 * iblb_set_tracers validates the positions as iblb_sample_points does, copies them, zeroes laps and
 * records t0 = iblb_get_step; stride >= 1.  It replaces any previous set; n == 0 removes the tracers, and
 * iblb_step is then exactly what it is without them.  A slab of a local or RCCL group: IBLB_ERR_UNSUPPORTED.
 * An error leaves the previous tracers as they were.
 * Update rule.  After the iterations t0 + stride, t0 + 2 stride, ... the context does one explicit-Euler
 * update with the state of that iteration held fixed: (ux, uy) = the bilinear sample above of IBLB_FIELD_UX and
 * IBLB_FIELD_UY at (x, y);  x' = x + (double)stride*ux,  y' = y + (double)stride*uy;  x' >= XDIM: x' -= XDIM,
 * laps += 1;  x' < 0: x' += XDIM, laps -= 1;  x' still outside [0, XDIM) after that one wrap: x and laps stay
 * as they were;  y' is clamped to [0, YDIM-1];  a non-finite ux or uy: the tracer keeps its position.  A stored
 * position is therefore always finite and in range, and a tracer's net x displacement is
 * x - x_start + laps*XDIM.
 * iblb_step(nsteps) with tracers cuts the call at the update iterations and schedules each piece (at most
 * `stride` iterations) as a call of its own; the result is by definition that of the caller doing
 * iblb_step(piece), sampling u and updating on the host.  Updates count on across calls: with stride 5,
 * iblb_step(3) then iblb_step(4) update once, after iteration t0 + 5.  A stride >= K (IBLB_SWEEP_DEPTH) keeps
 * the deep sweep between updates; stride 1 costs the one-step path at every iteration.  One update is one
 * launch, one lane per tracer, a gather of 36 population loads: tracers ordered like the lattice (y fastest)
 * share those loads between neighbouring lanes and update several times faster than tracers in random order
 * (DESIGN.md section 10).
 * iblb_set_state keeps the tracers (positions, laps and the update count) and re-bases t0 to the new state's
 * step count 0: the next update follows `stride` iterations later.  iblb_save_checkpoint does not hold the
 * tracers; iblb_save_checkpoint_ex does (IBLB_CKPT_TRACERS: positions, laps, the update count and the schedule).
 * iblb_load_checkpoint removes them and restores those its file holds. */
int iblb_set_tracers(iblb_ctx* ctx, long long n, const double* x, const double* y, int stride);
int iblb_get_tracers(iblb_ctx* ctx, double* x, double* y, int* laps);   /* [n] each; any may be NULL */
/* Tracers set, their stride and the updates done since iblb_set_tracers (any may be NULL). */
int iblb_tracer_count(iblb_ctx* ctx, long long* n, int* stride, long long* updates);

/* A motion model and a fate for the tracers: particles (a dust grain, a droplet, a bacterium) that the flow
 * carries, that jitter by Brownian motion, settle with a drift velocity and deposit on a wall.  On the device
 * the model adds status[n] in int and the hit iteration[n] in long long to the tracers' arrays; a context
 * without a model runs the plain update above, launch for launch. */
#define IBLB_TRACER_WALL_CLAMP   0   /* as the plain tracers: y clamped to the wall's row          */
#define IBLB_TRACER_WALL_REFLECT 1   /* specular: the overshoot is folded back                      */
#define IBLB_TRACER_WALL_ABSORB  2   /* the tracer deposits where its step crossed the wall's row   */
#define IBLB_TRACER_ALIVE     0
#define IBLB_TRACER_AT_BOTTOM 1
#define IBLB_TRACER_AT_TOP    2

typedef struct iblb_tracer_model {
    double diffusivity;          /* D >= 0, lattice units                              */
    double drift[2];             /* settling velocity added to the fluid's, finite     */
    int    wall[2];              /* IBLB_TRACER_WALL_* of the bottom [0] and top [1]   */
    unsigned long long seed;
} iblb_tracer_model;

/* iblb_set_tracer_model puts the model on the tracers currently set (m == NULL removes it; without one that is
 * IBLB_OK).  status0, iteration0 [n], both or neither: the fates to start from, as iblb_get_tracer_fates
 * returned them, so that a caller can put back the fates it read before a save and go on; both NULL: every
 * tracer alive.  The positions, laps, the schedule and the update count are those of the tracers and are not
 * touched.  No tracers set: IBLB_ERR_STATE.  A negative or non-finite diffusivity, a non-finite drift or an
 * unknown wall kind: IBLB_ERR_ARG, checked before anything is touched; only one of status0 / iteration0, a status
 * outside {0, 1, 2}, or a deposited status whose tracer's y is not on that wall's row (0, or YDIM-1):
 * IBLB_ERR_ARG.  Every error leaves the previous model and fates untouched.  (The hit iteration of an alive
 * tracer is stored as -1 whatever iteration0 holds for it.)
 * Update rule.  At the tracers' update iterations, for every tracer with status IBLB_TRACER_ALIVE; s =
 * (double)stride, m = the updates done before this one (iblb_tracer_count's `updates`), t = the iteration
 * (iblb_get_step), p = the tracer's index.  Double arithmetic throughout, one rounding per operation, no
 * contraction.
 *  1. (ux, uy) = the bilinear sample of the plain rule.  Non-finite: the tracer is unchanged and stays alive.
 *  2. Counter-based random numbers, so that a run cut into calls, restarted or re-based draws the same numbers;
 *     64-bit unsigned integers that wrap:
 *       mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *       key  = mix(seed + 0x9E3779B97F4A7C15 * (p + 1))
 *       r_k  = mix(key + 0x9E3779B97F4A7C15 * (2 m + k + 1)),  k = 0 for x, k = 1 for y
 *       xi_k = (double)(r_k >> 11) * 2^-52 - 1.0,  in [-1, 1) and exact
 *     The step is uniform, not Gaussian: its variance per update is amp^2 / 3 = 2 D stride, and the central
 *     limit theorem does the rest; no device log or cos appears whose last bits a host would not reproduce.
 *  3. amp = sqrt(6.0 * D * s), computed once on the host;
 *       xn = (x + s*(ux + drift[0])) + amp*xi_0,   yn = (y + s*(uy + drift[1])) + amp*xi_1
 *     (with D == 0 the random terms are skipped, which gives the same bits).
 *  4. Walls.  Bottom if yn < 0 (yw = 0), top if yn > YDIM-1 (yw = YDIM-1):
 *       CLAMP:    yn = yw
 *       REFLECT:  yn = -yn, respectively yn = yw - (yn - yw), then clamped into [0, YDIM-1]
 *       ABSORB:   lam = (yw - y)/(yn - y);  xn = x + lam*(xn - x);  yn = yw;  status = IBLB_TRACER_AT_BOTTOM /
 *                 IBLB_TRACER_AT_TOP, hit iteration = t
 *  5. x wraps with laps exactly as in the plain rule, on the final xn; still outside after one wrap: x and laps
 *     stay, y and the status still take effect.
 * So a deposited tracer never moves again, a stored position is always finite and in range, and a model with
 * D = 0, zero drift and both walls CLAMP gives the plain tracers bit for bit.
 * The model belongs to the tracer set it was put on: iblb_set_tracers (replace or remove) and iblb_load_checkpoint
 * remove it; iblb_set_state keeps it with the fates and the update count, as it keeps the tracers.  No checkpoint
 * holds the model or the fates: IBLB_CKPT_TRACERS writes the bytes it writes without a model.  A history under
 * IBLB_HIST_TRACERS records a deposited tracer's resting place again and again.
 * iblb_tracer_model_info: the model (zeroes without one), whether one is set, and counts[3] = the tracers alive,
 * at the bottom, at the top (zeroes without one); any may be NULL.
 * iblb_get_tracer_fates: status [n] and hit iteration [n] (-1 while alive), either may be NULL.
 * iblb_get_tracer_deposits: bottom [XDIM], top [XDIM], either may be NULL: the deposited tracers of each wall
 * per column floor(x), counted on the device (integer atomics: exact whatever the order), so that O(XDIM)
 * integers are copied out instead of the tracers.  Both without a model: IBLB_ERR_STATE. */
int iblb_set_tracer_model(iblb_ctx* ctx, const iblb_tracer_model* m,
                          const int* status0, const long long* iteration0);
int iblb_tracer_model_info(iblb_ctx* ctx, iblb_tracer_model* m, int* present, long long counts[3]);
int iblb_get_tracer_fates(iblb_ctx* ctx, int* status, long long* iteration);
int iblb_get_tracer_deposits(iblb_ctx* ctx, long long* bottom, long long* top);

/* Time- and phase-averaged fields: sums of chosen fields over a window that the context itself accumulates
 * on the device while iblb_step runs, so that a beat average (the mean flow, its fluctuation <u'u'>, the flow
 * at a given phase of the beat) needs no readback per sample and keeps the deep sweep between samples.
 * `w` and `fields` are those of iblb_get_fields (the IBLB_FIELD_* bits; NULL = the whole lattice at
 * stride 1); stride >= 1, nbins >= 1; flags: */
#define IBLB_AVG_SQ   1   /* also accumulate v*v of every requested field            */
#define IBLB_AVG_UXUY 2   /* also accumulate ux*uy (needs IBLB_FIELD_UX and _UY)      */
/* iblb_set_average validates its arguments, allocates zeroed accumulators on the device (per bin one plane of
 * w.ny * w.nx doubles per requested field, as many again under IBLB_AVG_SQ, one more under IBLB_AVG_UXUY) and
 * records t0 = iblb_get_step.  It replaces any previous set; fields == 0 with w == NULL removes averaging, and
 * iblb_step is then exactly what it is without it.  A bad window, fields == 0 with a window, an unknown field
 * bit or flag, IBLB_AVG_UXUY without both IBLB_FIELD_UX and IBLB_FIELD_UY, stride < 1 or nbins < 1:
 * IBLB_ERR_ARG, checked before anything is touched.  A slab of a local or RCCL group: IBLB_ERR_UNSUPPORTED.
 * Any error, IBLB_ERR_NOMEM included, leaves the previous set as it was.
 * Sampling rule.  After the iterations t0 + stride, t0 + 2 stride, ... the context takes sample number
 * m = 0, 1, 2, ... of the state of that iteration, and sample m goes to bin m % nbins: with stride * nbins equal
 * to the beat period, bin b holds the average at phase b.  For every window sample (i, j) and the k-th set bit of
 * `fields`, with v the value iblb_get_fields returns for that cell at that moment, bit for bit:
 *   sum = sum + v;   sum_sq = sum_sq + v*v  (IBLB_AVG_SQ);   sum_uxuy = sum_uxuy + ux*uy  (IBLB_AVG_UXUY)
 * in double, one rounding per operation, no contraction, in sample order; the bin's sample count goes up by
 * one.  Nothing is filtered: a non-finite v makes that cell's sums non-finite.  No summation is compensated.
 * iblb_step(nsteps) with averaging cuts the call at the sample iterations and schedules each piece (at most
 * `stride` iterations) as a call of its own; the result is by definition that of the caller doing
 * iblb_step(piece), then iblb_get_fields, then adding on the host.  Samples count on across calls.  With
 * tracers set as well the call is cut at the union of both event sets; at a common iteration both run (the
 * order of every observer: iblb_set_scalar below).  A scalar bit needs a scalar at the call (IBLB_ERR_STATE, the
 * previous set kept) and at every sample: iblb_set_scalar refuses to remove the scalar meanwhile, replacing it is
 * allowed and the average goes on with the new one.  A stride >= K (IBLB_SWEEP_DEPTH) keeps the deep sweep
 * between samples; stride 1 costs the one-step path at every iteration.  One sample is one launch on the
 * context's stream, one lane per window sample, without a host synchronise.
 * iblb_reset_average zeroes the sums and counts and sets t0 to the current step (the next sample is number 0,
 * `stride` iterations later); IBLB_ERR_STATE if no averaging is set.
 * iblb_get_average returns the raw sums of one bin and its sample count; means and variances are the caller's
 * division (mean = sum/samples, var = sum_sq/samples - mean^2), so that the result stays exactly checkable.
 * sum and sum_sq are [nf * w.ny * w.nx] in iblb_get_fields' layout, out[(k*ny + j)*nx + i]; sum_uxuy is
 * [w.ny * w.nx]; any of the pointers may be NULL.  A non-NULL pointer to a plane that was not requested
 * (sum_sq without IBLB_AVG_SQ, sum_uxuy without IBLB_AVG_UXUY) or a bin outside [0, nbins): IBLB_ERR_ARG, nothing
 * written.  No averaging set: IBLB_ERR_STATE.
 * iblb_average_info returns the window (resolved: NULL became the whole lattice), fields, stride, nbins, flags
 * and the samples taken since the set or the last reset (any pointer may be NULL); fields == 0: none set.
 * iblb_set_state keeps the accumulators and counts and re-bases t0 to the new state's step count 0: the next
 * sample follows `stride` iterations later.  iblb_save_checkpoint does not hold the averages;
 * iblb_save_checkpoint_ex does (IBLB_CKPT_AVERAGE: every bin and count and the schedule; with a scalar field only
 * together with IBLB_CKPT_SCALAR).  iblb_load_checkpoint removes averaging and restores what its file holds.
 * iblb_destroy frees the accumulators. */
int iblb_set_average(iblb_ctx* ctx, const iblb_window* w, unsigned fields, int stride, int nbins, unsigned flags);
int iblb_reset_average(iblb_ctx* ctx);
int iblb_get_average(iblb_ctx* ctx, int bin, double* sum, double* sum_sq, double* sum_uxuy, long long* samples);
int iblb_average_info(iblb_ctx* ctx, iblb_window* w, unsigned* fields, int* stride, int* nbins, unsigned* flags,
                      long long* samples_total);

/* History: time series at chosen points that the context itself records on the device while iblb_step runs, so
 * that the velocity at a probe over a beat, the concentration at a sensor over a release, or the paths the tracers
 * took need no readback per sample and keep the deep sweep between records.  The tracers, the averages and the
 * scalar hold the present moment or a sum over time; this observer keeps the sequence: a ring of `capacity`
 * records on the device, per-probe running statistics beside it, and any stretch of records back in one copy.
 * One history per context.  flags: */
#define IBLB_HIST_TRACERS 1   /* the positions are the context's tracers (pathlines) */
/* iblb_set_history without IBLB_HIST_TRACERS: x, y [n], n >= 1, are fixed probes, validated exactly as
 * iblb_sample_points validates them and copied to the device; `fields` is what iblb_sample_points accepts and must
 * not be 0 (IBLB_FIELD_VORT included: the observer runs on a lone slab only).  A record is np = popcount(fields)
 * planes of n doubles, plane k the k-th set bit (ascending).
 * With IBLB_HIST_TRACERS: x, y and n are ignored, the probes are the tracers set at the call (n = their count;
 * none set: IBLB_ERR_STATE), and `fields` may be 0, positions only.  Every record then starts with three more
 * planes before the field planes, x, y and (double)laps, so np = 3 + popcount(fields).  While such a history is
 * set iblb_set_tracers returns IBLB_ERR_STATE and changes nothing, whether it would replace or remove the
 * tracers: remove the history first.
 * Both: stride >= 1, capacity >= 1, no flag but the one above.  A negative n, a NULL x or y with n > 0, fields == 0
 * without the flag, an unknown field bit or flag, stride < 1, capacity < 1, YDIM < 2, or a point out of range or
 * non-finite: IBLB_ERR_ARG, checked before anything is touched.  A slab of a local or RCCL group:
 * IBLB_ERR_UNSUPPORTED.  A scalar bit (IBLB_FIELD_C, _CUX, _CUY) without a scalar: IBLB_ERR_STATE.  n == 0
 * without the flag removes the history (the other arguments are then not looked at, and a slab of a group may do
 * it too), and iblb_step is then exactly what it is without one.  A set replaces any previous history; the new
 * buffers are allocated before the old ones are freed, and any error, IBLB_ERR_NOMEM included, leaves the previous
 * history as it was.  A successful set starts `recorded` and the statistics at zero and records
 * t0 = iblb_get_step.  The ring takes capacity * np * n doubles on the device, the statistics 8 * np * n more.
 * Record rule.  After the iterations t0 + stride, t0 + 2 stride, ... the context takes record number
 * m = 0, 1, 2, ... of the state of that iteration into slot m % capacity of the ring; the iteration of each slot
 * is kept on the host.  Plane k at probe p holds the bits iblb_sample_points returns at that moment for that field
 * at that probe's position; under IBLB_HIST_TRACERS the three leading planes hold the bits iblb_get_tracers
 * returns and the field planes are sampled at those positions.  iblb_step(nsteps) with a history cuts the call at
 * the record iterations and schedules each piece (at most `stride` iterations) as a call of its own; the result is
 * by definition that of the caller doing iblb_step(piece), then iblb_sample_points (iblb_get_tracers), then
 * appending on the host.  Records count on across calls.  With other observers set the call is cut at the union
 * of the event sets, and at a common iteration the history runs last: the scalar's event, the tracers' update,
 * the averages' sample, then the record.  A pathline record therefore holds the positions after that iteration's
 * update, and a sample of C follows that iteration's event.  A scalar bit needs the scalar at every record:
 * iblb_set_scalar(cfg == NULL) returns IBLB_ERR_STATE meanwhile, replacing the scalar is allowed and the history
 * goes on with the new one.  A stride >= K (IBLB_SWEEP_DEPTH) keeps the deep sweep between records; stride 1
 * costs the one-step path at every iteration.  One record is one launch on the context's stream, one lane per
 * probe, without a host synchronise.
 * Running statistics, per plane and probe, updated by the same launch in record order, over every record since
 * the set or the last reset, those the ring has overwritten included.  In double, one rounding per operation, no
 * contraction, nothing compensated.  A finite v of record m:  count += 1;  sum = sum + v;  sum_sq = sum_sq + v*v;
 * v < min: min = v, min_rec = m;  v > max: max = v, max_rec = m.  A non-finite v only does nonfinite += 1.  With
 * nothing seen min = +inf, max = -inf and both record numbers are -1.
 * iblb_get_history returns the records [first, first + count) into out[((r*np) + k)*n + p], r counted from
 * `first`, and their iterations into iterations[r]; either pointer may be NULL, not both.  It needs
 * first >= max(0, recorded - capacity), count >= 0 and first + count <= recorded; otherwise IBLB_ERR_ARG and
 * nothing is written.  It does not drain the ring (a record stays until the ring overwrites it) and copies at
 * most two contiguous runs of it.
 * iblb_get_history_stats: every array is [np * n], index k*n + p; any pointer may be NULL, not all.
 * iblb_get_history_points returns the fixed probes, x [n] and y [n] (either may be NULL); under IBLB_HIST_TRACERS
 * IBLB_ERR_STATE (the positions are iblb_get_tracers').
 * iblb_reset_history zeroes `recorded` and the statistics, keeps the positions and the ring's size, and sets t0 to
 * the current step (the next record is number 0, `stride` iterations later).
 * iblb_history_info returns n, fields, stride, capacity, flags and the records taken since the set or the last
 * reset (any pointer may be NULL); no history set: n = 0 and the rest zero.  The getters and the reset then return
 * IBLB_ERR_STATE.
 * iblb_set_state keeps the history, its records and statistics, and re-bases t0 to the new state's step count 0:
 * the next record follows `stride` iterations later, and its iteration counts from the new state.  iblb_destroy
 * frees it.  No checkpoint holds a history, neither iblb_save_checkpoint nor iblb_save_checkpoint_ex (whose
 * observer bits stay the three they are): a caller drains the ring before saving and sets the history afresh after
 * loading.  iblb_load_checkpoint removes it, as it removes every observer.  A context that joins a group after the
 * set fails its next record with IBLB_ERR_UNSUPPORTED, as the scalar does. */
int iblb_set_history(iblb_ctx* ctx, long long n, const double* x, const double* y, unsigned fields, int stride,
                     long long capacity, unsigned flags);
int iblb_get_history(iblb_ctx* ctx, long long first, long long count, double* out, long long* iterations);
int iblb_get_history_stats(iblb_ctx* ctx, long long* count, long long* nonfinite, double* sum, double* sum_sq,
                           double* min, double* max, long long* min_rec, long long* max_rec);
int iblb_get_history_points(iblb_ctx* ctx, double* x, double* y);
int iblb_reset_history(iblb_ctx* ctx);
int iblb_history_info(iblb_ctx* ctx, long long* n, unsigned* fields, int* stride, long long* capacity,
                      unsigned* flags, long long* recorded);

/* Passive scalar: one concentration field C that the context itself advects with the fluid and diffuses while
 * iblb_step runs, so that transport and mixing (a solute cleared by the cilia, uptake at a wall) need neither a
 * readback of u per iteration nor a solver on the host.  A D2Q5 BGK advection-diffusion lattice: five populations
 * g_i per cell, stored in double whatever the context's precision; a lone slab only. */
#define IBLB_SCALAR_WALL_NOFLUX 0   /* halfway bounce-back: no flux through the wall      */
#define IBLB_SCALAR_WALL_VALUE  1   /* halfway anti-bounce-back: C = wall_value at the wall */
typedef struct iblb_scalar {
    double tau;            /* relaxation time, finite and > 0.5; diffusivity D = (tau - 0.5)/3 */
    int    stride;         /* >= 1: an event every `stride` iterations, `stride` substeps per event */
    int    wall_kind[2];   /* [0]: wall below row 0, [1]: wall above row YDIM-1 */
    double wall_value[2];  /* used (and required finite) where the kind is _VALUE */
} iblb_scalar;
/* iblb_set_scalar.  c0 is [N] in the reference layout (j = y*XDIM + x); g0 is [5N], plane-major g0[i*N + j], the
 * post-stream populations.  Exactly one of c0 and g0 must be non-NULL: with c0 the populations are the equilibrium
 * geq_i below at the ux, uy that iblb_get_fields returns at the call; g0 is taken as it is (a restart).  The call
 * records t0 = iblb_get_step and replaces any previous scalar; cfg == NULL (c0 and g0 ignored) removes the scalar,
 * and iblb_step is then exactly what it is without it.  tau not finite or <= 0.5, stride < 1, a wall kind other than
 * the two above, a non-finite wall value under _VALUE, both or neither of c0 and g0: IBLB_ERR_ARG, checked before
 * anything is touched.  A slab of a local or RCCL group: IBLB_ERR_UNSUPPORTED.  The new buffers are allocated
 * before the old ones are freed: any error, IBLB_ERR_NOMEM included, leaves the previous scalar as it was.
 * Update rule.  Directions i = 0..4 with c_i = (0,0), (+1,0), (-1,0), (0,+1), (0,-1); weights w0 = 1.0/3.0,
 * w1..4 = 1.0/6.0; omega = 1.0/tau, computed on the host in double.  An event runs after each of the iterations
 * t0 + stride, t0 + 2 stride, ...: it takes ux, uy of every cell as iblb_get_fields returns them at that moment,
 * bit for bit (in every phase, an owed IB force included), holds them fixed and does `stride` substeps, every
 * operation in double with one rounding and no contraction.  One substep, per cell:
 *   C     = (((g0 + g1) + g2) + g3) + g4
 *   a     = (0, ux, -ux, uy, -uy)
 *   geq_i = (w_i*C) * (1.0 + 3.0*a_i)
 *   p_i   = g_i - omega*(g_i - geq_i)
 *   g_i'(x, y) = p_i(x - c_ix, y - c_iy)                                  periodic in x
 *   g_3'(x, 0) = p_4(x, 0)                   no-flux wall below row 0;    _VALUE: (2.0*w1)*wall_value[0] - p_4(x, 0)
 *   g_4'(x, YDIM-1) = p_3(x, YDIM-1)         no-flux wall above the top;  _VALUE: (2.0*w1)*wall_value[1] - p_3(x, YDIM-1)
 * Nothing is filtered: a non-finite value spreads.  The scheme conserves sum(C) between no-flux walls, and diffuses
 * with D = (tau - 0.5)/3 (its error grows towards tau = 0.5 and with the cell Peclet number |u|/D).
 * iblb_step(nsteps) with a scalar cuts the call at the union of the scalar's, the tracers' and the averages' event
 * sets; at a common iteration all due observers run: the scalar's event first, then the tracers' update and the
 * averages' sample, so that a sample of IBLB_FIELD_C / _CUX / _CUY sees C after that iteration's event (for every
 * other field the order cannot be observed: no observer changes the fluid state).  cfg == NULL while the current
 * average holds a scalar bit: IBLB_ERR_STATE, nothing changed (remove or replace the average first).  A
 * stride >= K (IBLB_SWEEP_DEPTH) keeps the deep sweep between events; stride 1 costs the one-step path at every
 * iteration.  A substep is one launch on the context's stream, one lane per cell, 96 bytes per cell, without a host
 * synchronise.
 * iblb_get_scalar returns C = (((g0+g1)+g2)+g3)+g4 of the stored populations on the window into c[j*w.nx + i]
 * (the window rules of iblb_get_fields; NULL = the whole lattice).  No scalar set: IBLB_ERR_STATE; a bad window or
 * c == NULL: IBLB_ERR_ARG, no output touched.  iblb_get_scalar_populations returns g [5N] in the layout of g0.
 * iblb_scalar_info returns the configuration and the events run since the set (either pointer may be NULL);
 * cfg->stride == 0: no scalar is set.
 * iblb_set_state keeps the scalar (populations and event count) and re-bases t0 to the new state's step count 0.
 * iblb_save_checkpoint does not hold the scalar; iblb_save_checkpoint_ex does (IBLB_CKPT_SCALAR: the populations,
 * the event count and the schedule, and its source, uptake, ends and gauges).  iblb_load_checkpoint removes the scalar
 * and restores the one its file holds.  A context that joins a group after the set fails its
 * next event with IBLB_ERR_UNSUPPORTED.  iblb_destroy frees the scalar.
 * iblb_get_scalar_wall_flux.  bottom[x], top[x], x < XDIM (either may be NULL, not both): the net amount of C that
 * entered column x through that wall during the last substep, from the stored populations:
 *   _VALUE:  bottom[x] = 2.0*g3(x,0) - (2.0*w1)*wall_value[0];  top[x] = 2.0*g4(x,YDIM-1) - (2.0*w1)*wall_value[1]
 *   _NOFLUX: 0.0 exactly.   w1 = 1.0/6.0.   Before any substep it is merely this expression of g0.
 * (Anti-bounce-back stores g3' = 2 w1 Cw - p4: what entered minus what left is g3' - p4 = 2 g3' - 2 w1 Cw, so the
 * sum over x of bottom + top is the change of sum(C) over that substep up to rounding.)
 * No scalar: IBLB_ERR_STATE; both NULL: IBLB_ERR_ARG. */
int iblb_set_scalar(iblb_ctx* ctx, const iblb_scalar* cfg, const double* c0, const double* g0);
int iblb_get_scalar(iblb_ctx* ctx, const iblb_window* w, double* c);
int iblb_get_scalar_populations(iblb_ctx* ctx, double* g);
int iblb_scalar_info(iblb_ctx* ctx, iblb_scalar* cfg, long long* updates);
int iblb_get_scalar_wall_flux(iblb_ctx* ctx, double* bottom, double* top);

/* The scalar's source: what enters and leaves C other than through a wall held at one uniform value.  A bulk source
 * per cell, a first-order decay, a prescribed flux per column through a no-flux wall, and a wall value per column at
 * a _VALUE wall; each costs no readback and keeps the deep sweep. */
typedef struct iblb_scalar_source {
    const double* source;         /* [N], j = y*XDIM + x: amount of C added to the cell per substep; NULL = 0 */
    double        decay;          /* k: finite, >= 0; first-order loss per substep                            */
    const double* wall_flux[2];   /* [XDIM] each, only where the scalar's wall kind is _NOFLUX: amount of C
                                     entering column x through that wall per substep (negative: leaving);
                                     NULL = 0, the no-flux wall                                               */
    const double* wall_value[2];  /* [XDIM] each, only where the wall kind is _VALUE: the wall value of
                                     column x in place of iblb_scalar.wall_value[k]; NULL = the uniform one   */
} iblb_scalar_source;             /* [0]: wall below row 0, [1]: wall above row YDIM-1 */
/* iblb_set_scalar_source needs a scalar (IBLB_ERR_STATE otherwise; that covers the slabs of a group, which cannot
 * hold one).  It copies its arrays to the device, replaces any previous source and takes effect from the next
 * substep that runs; it moves neither t0 nor the event count.  src == NULL removes the source.  decay not finite or
 * negative, a non-finite entry in any array, wall_flux[k] given for a _VALUE wall, wall_value[k] given for a _NOFLUX
 * wall: IBLB_ERR_ARG, checked before anything is touched.  The new device buffers are allocated before the old ones
 * are freed: any error, IBLB_ERR_NOMEM included, leaves the previous source as it was.
 * Update rule.  With a source set, one substep replaces the relaxation line and the two wall lines of the rule of
 * iblb_set_scalar by (every operation in double, rounded once, no contraction):
 *   m   = decay*C
 *   r   = s(x,y) - m                                          s = 0.0 where `source` is NULL
 *   p_i = (g_i - omega*(g_i - geq_i)) + w_i*r
 *   g_3'(x, 0)      = p_4(x, 0) + wall_flux[0][x]             _NOFLUX (0.0 where NULL)
 *                   = (2.0*w1)*wall_value[0][x] - p_4(x, 0)   _VALUE  (the uniform value where NULL)
 *   g_4'(x, YDIM-1) = likewise with p_3 and index [1]
 * The rule is applied in full whenever a source is set: no term is skipped for a NULL array or for decay == 0, so
 * results are pinned by value (==); the sign of a zero is not part of the contract.  With no source set the substep
 * is exactly the rule of iblb_set_scalar.  Between walls of kind _NOFLUX sum(C) changes per substep by
 * sum(r) + sum_x(wall_flux[0][x] + wall_flux[1][x]), up to rounding.  A substep with a source reads one more plane:
 * 104 bytes per cell.
 * iblb_get_scalar_wall_flux with a source set: a _NOFLUX wall returns wall_flux[k][x] exactly (0.0 where NULL), a
 * _VALUE wall uses wall_value[k][x] in its expression.
 * iblb_set_scalar removes the source with the scalar it belonged to, whether it replaces or removes the scalar (a
 * replacement may change the wall kinds: set the source again).  iblb_set_state keeps the source,
 * iblb_load_checkpoint removes it along with the scalar (iblb_save_checkpoint does not hold the source;
 * iblb_save_checkpoint_ex does, with the scalar, and the load then restores it), iblb_destroy frees it.
 * iblb_scalar_source_info (either pointer may be NULL): decay, and present = 1 (a source is set) | 2 (`source`)
 * | 4, 8 (wall_flux[0], [1]) | 16, 32 (wall_value[0], [1]); no source set: 0 and 0.0.
 * iblb_get_scalar_source returns `source` [N] in the reference layout, zeros where the source was set without it.
 * No source set: IBLB_ERR_STATE; source == NULL: IBLB_ERR_ARG. */
int iblb_set_scalar_source(iblb_ctx* ctx, const iblb_scalar_source* src);
int iblb_scalar_source_info(iblb_ctx* ctx, double* decay, unsigned* present);
int iblb_get_scalar_source(iblb_ctx* ctx, double* source);

/* The scalar's uptake: first-order absorption at the no-flux walls (a reactive wall: the flux out of a column is its
 * rate times C at the wall), and per-column accumulators of what crossed each wall, whatever the wall's kind, updated
 * by every substep on the device.  It costs no readback and keeps the deep sweep; with no uptake set nothing changes. */
typedef struct iblb_scalar_uptake {
    const double* rate[2];   /* [XDIM] each, only where the scalar's wall kind is _NOFLUX: k[x], finite, >= 0,
                                flux out of column x = k[x] * C at the wall, per substep; NULL = 0 */
} iblb_scalar_uptake;        /* [0]: wall below row 0, [1]: wall above row YDIM-1 */
/* iblb_set_scalar_uptake needs a scalar (IBLB_ERR_STATE otherwise; that covers the slabs of a group, which cannot
 * hold one).  It copies its arrays to the device, replaces any previous uptake and takes effect from the next
 * substep that runs; it moves neither t0 nor the event count.  up == NULL removes the uptake.  A struct with both
 * rates NULL is valid: it only accumulates.  A rate entry that is not finite or is negative, rate[k] given for a
 * _VALUE wall: IBLB_ERR_ARG, checked before anything is touched.  The new device buffers are allocated before the old
 * ones are freed: any error, IBLB_ERR_NOMEM included, leaves the previous uptake (rates, totals, substeps) as it
 * was.  A successful set, a replacement included, starts total, last and substeps at zero.
 * Update rule.  On the host, once per set (every operation in double, rounded once, no contraction):
 *   a_k[x] = 2.0 - 2.0/(1.0 + 3.0*rate[k][x])                 0.0 where rate[k] is NULL
 * With an uptake set, one substep replaces the wall line of the rule in force (that of iblb_set_scalar, or of
 * iblb_set_scalar_source when a source is set) by the following, for the wall below row 0; the wall above the top row
 * likewise with p_3(x, YDIM-1), g_4'(x, YDIM-1) and index [1].  q = p_4(x, 0), the relaxed population of the rule in
 * force (with the source's w_i*r term when a source is set); e = wall_flux[0][x] of a set source, else 0.0:
 *   _NOFLUX:  l = a_0[x]*q;   g_3'(x, 0) = (q - l) + e;   net = e - l
 *   _VALUE:   g_3'(x, 0) as the rule in force (unchanged);   net = g_3'(x, 0) - q
 *   total[0][x] = total[0][x] + net;   last[0][x] = net;   substeps = substeps + 1 (once per substep)
 * Every operation in double, rounded once, no contraction; no term is skipped for a NULL array, so results are pinned
 * by value (==); the sign of a zero is not part of the contract.  net is what entered column x through that wall
 * during the substep (negative: left).  Halfway anti-bounce-back gives p_4 + g_3' = 2 w1 C_w; with g_3' = (1 - a) p_4
 * the loss a p_4 equals k C_w for a = 6k/(1 + 3k) = 2 - 2/(1 + 3k): a runs from 0 (the no-flux wall) to 2 as k grows,
 * and a = 2 is exactly the _VALUE wall at 0.0.  The steady state between such a wall and a _VALUE wall is exact.
 * Between walls that are not _VALUE and with no bulk source or decay, sum(C) changes per substep by
 * sum_x(net bottom + net top), up to rounding.  An event of `stride` substeps adds every one of them; each entry has
 * one writer per substep and the substeps are ordered, so the sums are reproducible bit for bit.
 * iblb_get_scalar_wall_flux keeps its stated expressions under an uptake: at a _NOFLUX wall it returns the prescribed
 * flux (or 0.0) and does not contain the uptake loss; last_bottom / last_top below are the full net.
 * iblb_get_scalar_uptake returns total and last of both walls, [XDIM] each, and the substeps accumulated; any pointer
 * may be NULL, not all five (IBLB_ERR_ARG).  iblb_reset_scalar_uptake zeroes total, last and substeps and keeps the
 * rates.  No uptake set: IBLB_ERR_STATE from both.
 * iblb_scalar_uptake_info (either pointer may be NULL): present = 1 (an uptake is set) | 2, 4 (rate[0], rate[1]), and
 * substeps; none set: 0 and 0.
 * iblb_set_scalar removes the uptake with the scalar it belonged to, whether it replaces or removes the scalar.
 * iblb_set_scalar_source keeps the uptake and its totals, setting or removing the source.  iblb_set_state keeps it,
 * iblb_load_checkpoint removes it along with the scalar (iblb_save_checkpoint does not hold the uptake;
 * iblb_save_checkpoint_ex does, with the scalar: the derived coefficients, total, last and substeps, and the load then
 * restores them), iblb_destroy frees it. */
int iblb_set_scalar_uptake(iblb_ctx* ctx, const iblb_scalar_uptake* up);
int iblb_get_scalar_uptake(iblb_ctx* ctx, double* total_bottom, double* total_top, double* last_bottom,
                           double* last_top, long long* substeps);
int iblb_reset_scalar_uptake(iblb_ctx* ctx);
int iblb_scalar_uptake_info(iblb_ctx* ctx, unsigned* present, long long* substeps);

/* The scalar's open ends in x.  The scalar is periodic in x because the fluid is: what leaves through column XDIM-1
 * comes back in at column 0.  With ends set nothing wraps: each end in x has a kind, no flux, a value per row (an
 * inlet profile) or a zero-gradient outflow, and per-row accumulators record what crossed each end, updated by every
 * substep on the device.  It costs no readback and keeps the deep sweep; with no ends set nothing changes.  The fluid
 * stays periodic. */
#define IBLB_SCALAR_END_NOFLUX  0   /* halfway bounce-back: nothing crosses the end               */
#define IBLB_SCALAR_END_VALUE   1   /* halfway anti-bounce-back: C = value at the end (an inlet)  */
#define IBLB_SCALAR_END_OUTFLOW 2   /* zero-gradient: the missing population is the cell's own    */
typedef struct iblb_scalar_ends {
    int           kind[2];     /* [0]: the end left of column 0, [1]: the end right of column XDIM-1 */
    double        value[2];    /* uniform value of a _VALUE end; required finite there               */
    const double* profile[2];  /* [YDIM] each, only at a _VALUE end: the value of row y in place of
                                  value[k]; NULL = the uniform one                                   */
} iblb_scalar_ends;
/* iblb_set_scalar_ends needs a scalar (IBLB_ERR_STATE otherwise; that covers the slabs of a group, which cannot hold
 * one).  It copies its arrays to the device, replaces any previous ends and takes effect from the next substep that
 * runs; it moves neither t0 nor the event count.  ends == NULL removes them: the scalar is periodic again, exactly
 * the rule in force.  A kind outside the three, a value[k] that is not finite at a _VALUE end, profile[k] given at an
 * end that is not _VALUE, a profile entry that is not finite: IBLB_ERR_ARG, checked before anything is touched.  The
 * new device buffers are allocated before the old ones are freed: any error, IBLB_ERR_NOMEM included, leaves the
 * previous ends (kinds, values, totals, substeps) as they were.  A successful set, a replacement included, starts
 * total, last and substeps at zero.
 * Update rule.  With ends set, one substep replaces only the x-streaming of the populations 1 and 2 at the two end
 * columns; everything else stays as the rule in force has it (that of iblb_set_scalar, of iblb_set_scalar_source, of
 * iblb_set_scalar_uptake): the relaxation, the walls, the uptake, and the streaming between the columns 0 .. XDIM-1.
 * p_i is the relaxed population of the rule in force (with the source's w_i*r term when a source is set).  At x = 0:
 * q = p_2(0, y) would leave through the left end, g_1'(0, y) has no source cell, and v = profile[0][y], or value[0]
 * where profile[0] is NULL:
 *   _NOFLUX:   g_1'(0, y) = q
 *   _VALUE:    g_1'(0, y) = (2.0*w1)*v - q
 *   _OUTFLOW:  g_1'(0, y) = p_1(0, y)           (what column 1 receives: g_1'(0, y) == g_1'(1, y))
 *   net = g_1'(0, y) - q
 *   total[0][y] = total[0][y] + net;   last[0][y] = net;   substeps = substeps + 1 (once per substep)
 * At x = XDIM-1 likewise with q = p_1(XDIM-1, y), the target g_2'(XDIM-1, y), p_2(XDIM-1, y) for _OUTFLOW, and index
 * [1].  Nothing wraps: p_1(XDIM-1, y) and p_2(0, y) reach no other column.  XDIM == 1 is valid: that one column has
 * both ends.  Every operation in double, rounded once, no contraction; no term is skipped, so results are pinned by
 * value (==); the sign of a zero is not part of the contract.  net is the amount of C that entered row y through that
 * end during the substep (negative: it left).  D2Q5 has no diagonal links, so at a corner cell the wall rule and the
 * end rule concern different directions and never meet; the streaming map stays a bijection of (cell, direction).
 * Between walls that are not _VALUE, and with no bulk source or decay, sum(C) changes per substep by the nets of both
 * ends plus the nets of both walls (iblb_get_scalar_uptake), up to rounding.  An event of `stride` substeps adds every
 * one of them; each entry has one writer per substep and the substeps are ordered, so the sums are reproducible bit
 * for bit.
 * iblb_get_scalar_ends returns total and last of both ends, [YDIM] each, and the substeps accumulated; any pointer may
 * be NULL, not all five (IBLB_ERR_ARG).  iblb_reset_scalar_ends zeroes total, last and substeps and keeps the kinds
 * and values.  No ends set: IBLB_ERR_STATE from both.
 * iblb_scalar_ends_info (any pointer may be NULL): kind and value as given, present = 1 (ends are set) | 2, 4
 * (profile[0], profile[1]), and substeps; none set: present 0, substeps 0, kind and value untouched.
 * iblb_set_scalar removes the ends with the scalar they belonged to, whether it replaces or removes the scalar.
 * iblb_set_scalar_source and iblb_set_scalar_uptake keep the ends and their totals, and iblb_set_scalar_ends keeps
 * the source and the uptake with its totals.  iblb_set_state keeps them, iblb_load_checkpoint removes them along with
 * the scalar (iblb_save_checkpoint does not hold the ends; iblb_save_checkpoint_ex does, with the scalar: kinds, values,
 * total, last and substeps, and the load then restores them), iblb_destroy frees them.
 * The readers are untouched: iblb_get_scalar_wall_flux and the uptake keep their expressions, and iblb_sample_points
 * still interpolates between column XDIM-1 and column 0, which is the fluid's periodicity and is not meaningful for C
 * (IBLB_FIELD_C, _CUX) under open ends: sample C at 0 <= x <= XDIM-1 there. */
int iblb_set_scalar_ends(iblb_ctx* ctx, const iblb_scalar_ends* ends);
int iblb_get_scalar_ends(iblb_ctx* ctx, double* total_left, double* total_right, double* last_left,
                         double* last_right, long long* substeps);
int iblb_reset_scalar_ends(iblb_ctx* ctx);
int iblb_scalar_ends_info(iblb_ctx* ctx, int kind[2], double value[2], unsigned* present, long long* substeps);

/* The scalar's transport gauges.  The walls and the ends record what leaves the lattice; gauges record what moves
 * inside it: across the links between chosen columns and their right neighbours (stations) and between chosen rows and
 * the rows above them (levels), advection and diffusion together, summed over every substep on the device.  They cost
 * no readback and keep the deep sweep; they change no population, and with none set nothing changes. */
typedef struct iblb_scalar_gauges {
    int n_stations; const int* station;  /* station k: the link between column station[k] and the column to its right */
    int n_levels;   const int* level;    /* level k: the link between row level[k] and row level[k]+1 */
} iblb_scalar_gauges;
/* iblb_set_scalar_gauges needs a scalar (IBLB_ERR_STATE otherwise; that covers the slabs of a group, which cannot hold
 * one).  It copies its arrays, replaces any previous gauges and takes effect from the next substep that runs; it moves
 * neither t0 nor the event count.  gauges == NULL removes them.  0 <= n_stations <= XDIM and 0 <= n_levels <= YDIM-1,
 * not both 0; the entries strictly ascending with 0 <= station[k] <= XDIM-1 and 0 <= level[k] <= YDIM-2; an array is
 * NULL only where its count is 0.  Anything else: IBLB_ERR_ARG, checked before anything is touched.  The new device
 * buffers are allocated before the old ones are freed: any error, IBLB_ERR_NOMEM included, leaves the previous gauges
 * (positions, totals, substeps) as they were.  A successful set, a replacement included, starts the totals and
 * substeps at zero.
 * Update rule.  p_i is the relaxed population of the rule in force (with the source's w_i*r term when a source is
 * set), the p_i the ends' rule names.  With gauges set, one substep also does, for station k at column
 * X = station[k] and every row y,
 *   right[k][y] = right[k][y] + p_1(X, y)        (what leaves column X towards +x)
 *   left[k][y]  = left[k][y]  + p_2(X+1, y)      (what leaves the column right of X towards -x)
 * where, the scalar periodic, the column right of XDIM-1 is column 0 (XDIM == 1 is valid: the one column feeds both
 * entries); with ends set (iblb_set_scalar_ends) there is no link right of column XDIM-1 and a station there adds 0.0
 * to both entries.  For level k at row Y = level[k] and every column x,
 *   up[k][x]   = up[k][x]   + p_3(x, Y)
 *   down[k][x] = down[k][x] + p_4(x, Y+1)
 * and substeps = substeps + 1, once per substep.  Every operation in double, rounded once, no contraction: results
 * are pinned by value (==); the sign of a zero is not part of the contract.  The net amount that crossed a station
 * towards +x is right - left, a level towards +y up - down; the subtraction is the caller's.  The gauges change no
 * population: with gauges set the scalar, the uptake's totals and the ends' totals are bit for bit what they are
 * without.  Each entry has one writer per substep and the substeps are ordered, so the totals are reproducible bit for
 * bit.  The change of sum(C) over any box of columns (X0, X1] and rows (Y0, Y1] is the nets of the four gauges on its
 * sides (walls' and ends' totals where a side is a wall or an end, the box's sum of r with a source), up to rounding.
 * iblb_get_scalar_gauges returns right and left, [n_stations*YDIM] each, index k*YDIM + y, up and down,
 * [n_levels*XDIM] each, index k*XDIM + x, and the substeps accumulated; any pointer may be NULL, not all five
 * (IBLB_ERR_ARG); an array whose count is 0 is left untouched.  iblb_reset_scalar_gauges zeroes the totals and
 * substeps and keeps the positions.  No gauges set: IBLB_ERR_STATE from both.
 * iblb_scalar_gauges_info (any pointer may be NULL): the counts, the positions as given (station and level must hold
 * what the counts say: ask for the counts first), and substeps; none set: counts 0, substeps 0, arrays untouched.
 * iblb_set_scalar removes the gauges with the scalar they belonged to, whether it replaces or removes the scalar.
 * iblb_set_state, iblb_set_scalar_source, iblb_set_scalar_uptake and iblb_set_scalar_ends keep them with their totals,
 * and iblb_set_scalar_gauges keeps the source, the uptake and the ends with their totals.  iblb_load_checkpoint
 * removes them along with the scalar (iblb_save_checkpoint does not hold the gauges; iblb_save_checkpoint_ex does, with
 * the scalar: the positions, the four totals and substeps, and the load then restores them), iblb_destroy frees them. */
int iblb_set_scalar_gauges(iblb_ctx* ctx, const iblb_scalar_gauges* gauges);
int iblb_get_scalar_gauges(iblb_ctx* ctx, double* right, double* left, double* up, double* down, long long* substeps);
int iblb_reset_scalar_gauges(iblb_ctx* ctx);
int iblb_scalar_gauges_info(iblb_ctx* ctx, int* n_stations, int* station, int* n_levels, int* level,
                            long long* substeps);

/* Timing: when enabled (1) every collide-stream launch is bracketed by HIP events on the
 * stream it runs on; iblb_get_timing() returns the sums (and resets them if reset).  enabled = 2:
 * only the deep (K-iteration) launches are timed, by their own dispatch / completion signals (no
 * marker packets; the IB band cycle's chain launches run untimed), so that a timed region with IB
 * keeps its schedule. */
int iblb_set_profiling(iblb_ctx* ctx, int enabled);
int iblb_get_timing(iblb_ctx* ctx, iblb_timing* t, int reset);
/* The same, writing at most `bytes` bytes of the struct (pass sizeof(iblb_timing) of the header the
 * caller was built with: an older, shorter iblb_timing gets its own fields only).  iblb_get_timing
 * writes sizeof(iblb_timing) of THIS header. */
int iblb_get_timing_ex(iblb_ctx* ctx, iblb_timing* t, unsigned long bytes, int reset);
/* The collide build of the context's last deep launch (the one iblb_timing's deep_mode ... deep_vgprs
 * name): 1 the build for a body force along x only (F_y = 0: the same populations bit for bit, fewer
 * operations), 0 the general one (F_y != 0, a build without the x-only variant, or IBLB_DEEP_FORCE=general),
 * -1 no deep launch yet (or ctx NULL).  No struct changed for it: the ABI version stays. */
int iblb_deep_force_build(const iblb_ctx* ctx);
/* The stream the context launches on (hipStream_t), for callers that add work. */
int iblb_get_stream(iblb_ctx* ctx, void** stream);
/* Block until all work of the context is done. */
int iblb_synchronize(iblb_ctx* ctx);

/* ---- x-slab decomposition -------------------------------------------------------
 * Slabs are ordered along x (periodic).  Every population buffer of a slab holds ghost
 * columns on both sides (3K per side, K = IBLB_SWEEP_DEPTH); a halo exchange of depth d
 * sends the d whole edge columns of the current state to each neighbour and receives the
 * neighbours' into the ghost columns, in place (no packing): d = 1 for a one-step
 * iteration, 3 when an owed IB force is evaluated from the ghosts, K per K-iteration deep
 * cycle, 3K per IB band cycle whose trapezoids cross a slab edge.
 *
 * Local group: n contexts of ONE process (any devices with peer access) linked
 * left-to-right; iblb_group_step() advances them together.  Synchronous transport,
 * meant for testing the decomposition on one GPU.
 *
 * RCCL group: one context per process; rank 0 creates the id, it is broadcast by the
 * caller (e.g. torch.distributed), every rank attaches; iblb_step() then exchanges
 * halos with ncclSend/ncclRecv on a second stream, overlapped with the collide of the
 * interior columns (IBLB_OVERLAP=0 in the environment selects the sequential schedule).
 * With an RCCL group iblb_step, iblb_set_lagrangian and every reader are collective. */
int iblb_link_local(iblb_ctx** ctxs, int n);
int iblb_group_step(iblb_ctx** ctxs, int n, int nsteps);
int iblb_rccl_unique_id(char id[IBLB_UNIQUE_ID_BYTES]);
int iblb_attach_rccl(iblb_ctx* ctx, const char id[IBLB_UNIQUE_ID_BYTES], int nranks, int rank);
/* Bound of the RCCL group's device-side waits, in seconds of wall-clock time (default 600, or
 * IBLB_WAIT_TIMEOUT_S from the environment at iblb_create).  Inside a run of deep cycles a slab's
 * kernels wait for the boundary work of the previous cycle on a device word rather than in the
 * hardware queue; that work follows the cycle's halo exchange, i.e. the neighbour ranks.  A rank
 * whose host reaches its next iblb_step late (writing output, a checkpoint, the caller's own work)
 * delays those waits like RCCL's own kernels and changes no result; only a wait longer than this
 * bound fails: the iblb_step / iblb_synchronize that sees it returns IBLB_ERR_COMM and the state
 * must be set again.  Set it at least as long as the longest pause any rank takes between calls. */
int iblb_set_wait_timeout(iblb_ctx* ctx, double seconds);

/* Whole-lattice rho [nx*ny] and u [2*nx*ny] (reference layout, j = y*XDIM + x) on rank `root`
 * of an RCCL group: the output gather the reference's single-GPU BigData writer needs
 * (main.cu:938-971) when the lattice is split over GPUs.  Collective; the other ranks may
 * pass NULL.  A single slab returns iblb_get_macro. */
int iblb_gather_macro(iblb_ctx* ctx, int root, double* rho, double* u);

/* ---- checkpoint / restart (absent in the reference; its jobs run 1e5+ steps, cilia6.sh) --
 * iblb_save_checkpoint writes this context's slab: the stored populations in their storage
 * precision, step count, cumulative flux Q, Lagrangian points and cilia kinematics state
 * (written to path.tmp, then renamed).  iblb_load_checkpoint restores it into a context
 * created with the same lattice, slab, precision, tau/tau2 and body force (and enough
 * max_points); stepping on from there is bit-identical to the uninterrupted run up to the
 * summation order of the IB spread.  Each rank of a group saves / loads its own file;
 * restore before iblb_link_local, before or after iblb_attach_rccl. */
int iblb_save_checkpoint(iblb_ctx* ctx, const char* path);
int iblb_load_checkpoint(iblb_ctx* ctx, const char* path);

/* Checkpoints that hold the observers as well.  iblb_save_checkpoint holds the fluid alone, and loading such a
 * file removes the tracers, the averages and the scalar.  iblb_save_checkpoint_ex writes exactly the bytes of
 * iblb_save_checkpoint and then one section for every observer that `observers` (IBLB_CKPT_* bits) asks for and
 * that is set, closed by an end section:
 *   IBLB_CKPT_SCALAR   the scalar as given, its event schedule and populations, and with it its source (decay,
 *                      field, wall arrays), its uptake (the derived coefficients, total, last, substeps), its ends
 *                      (kinds, values, the rows' values, total, last, substeps) and its gauges (positions, the four
 *                      totals, substeps);
 *   IBLB_CKPT_TRACERS  n, stride, the update count, x, y and laps;
 *   IBLB_CKPT_AVERAGE  the resolved window, fields, stride, nbins, flags, the sample counts and every plane of
 *                      every bin.
 * A requested observer that is not set writes no section (no error); when no section results — observers == 0,
 * nothing set, a slab of a group, which holds no observer — the file is byte for byte iblb_save_checkpoint's, with
 * no end section.  An unknown bit: IBLB_ERR_ARG.  IBLB_CKPT_AVERAGE without IBLB_CKPT_SCALAR while the current
 * average holds IBLB_FIELD_C, _CUX or _CUY: IBLB_ERR_ARG (such a file could not be restored).  Before the first
 * step: IBLB_ERR_STATE, as iblb_save_checkpoint.  On any error no file appears at path and path.tmp is removed.
 * The file does not depend on the device's layouts; its format is described in csrc/ckpt_format.h (the framing)
 * and above the checkpoint code of csrc/iblb_ctx.hip (the payloads).
 *
 * iblb_load_checkpoint takes both kinds of file.  It removes the three observers and then restores those the file
 * holds: every *_info call and every getter then returns what it returned at the save, and stepping on gives what
 * the uninterrupted run gives — populations, totals, last, substeps, positions, laps, bins and counts, bit for bit
 * where the fluid restart is (no IB points).  The schedules go on by absolute iteration: a scalar of stride 3 set
 * at iteration 0 and saved at iteration 7 has its next event after iteration 9.  The whole observer part is
 * checked before anything is touched — the framing (known tags in order, lengths that fit the file, an end section
 * and nothing behind it) and every section against the context (array sizes against XDIM and YDIM, positions and
 * windows in range, wall and end kinds, stride >= 1, tau finite and > 0.5, a scalar field in the average only with
 * a scalar section): a malformed, truncated or inconsistent observer part returns IBLB_ERR_ARG and leaves the
 * context exactly as it was.  A file with an observer part loaded into a context attached to an RCCL group returns
 * IBLB_ERR_UNSUPPORTED, equally before anything is touched.  A HIP or allocation failure during the restore leaves
 * the context as any failed load does: empty (it needs a state or another load), without observers.
 *
 * iblb_checkpoint_info reads the fluid header and the framing of a file: the step count and the IBLB_CKPT_* bits
 * of the sections present (either pointer may be NULL).  It needs no context and no device, and returns
 * IBLB_ERR_ARG where iblb_load_checkpoint would refuse the file's framing. */
#define IBLB_CKPT_SCALAR    1   /* the scalar with its source, uptake, ends and gauges, totals included */
#define IBLB_CKPT_TRACERS   2
#define IBLB_CKPT_AVERAGE   4
#define IBLB_CKPT_OBSERVERS 7
int iblb_save_checkpoint_ex(iblb_ctx* ctx, const char* path, unsigned observers);
int iblb_checkpoint_info(const char* path, long long* step, unsigned* observers);

#ifdef __cplusplus
}
#endif
#endif /* IBLB_H */
