// ctx.h — the context of the fused C ABI (include/iblb.h part 2) and the host helpers shared by
// its translation units:
//   iblb_ctx.hip   lifecycle, state, Lagrangian points, timing, checkpoint / restart (the files' framing:
//                  ckpt_format.h, pure host code checked on the CPU)
//   ctx_read.hip   the readers: the current state to the host in the reference layouts, windowed
//                  fields and reductions, point sampling, the output gather
//   ctx_observe.hip  what iblb_step runs between the pieces of a call: passive tracers, averaged fields,
//                  the passive scalar, the history recorder
//   ctx_step.hip   halo exchange, the one-step / two-step / deep schedules, iblb_step, local and
//                  RCCL groups
//   ctx_band.hip   the IB band cycle (K iterations per cycle with an owed force every iteration)
// Every reader and observer is built from the read scaffold below (with_state ... read_back).
//   band_plan.h    the band cycle's planner: pure host functions (no HIP), checked on the CPU
//   deep_plan.h    the deep sweep's launch planner (builds, sweeps, edge waves, a call's depths,
//                  IBLB_DEEP_BUILD): pure host functions too, applied by lbm_sweep_impl.h's launchers
//
// Time-step bookkeeping.  The reference iteration (main.cu:852-909) is
//   f0,F = equilibrium(u^t, rho^t, force^t); f1 = collision(f^t); f^{t+1} = stream(f1);
//   rho^{t+1}, u_raw = macro(f^{t+1}); F_s = interpolate(...); force^{t+1}, u^{t+1} = spread(...)
// The context stores g = f1^{t-1} (post-collision, not yet streamed).  One fused launch pulls f^t
// from g, recomputes rho^t and u^t = (sum c f + force^t/2)/rho^t, collides and stores f1^t.
// force^t (the IB part of the PREVIOUS reference iteration) is computed lazily just before it is
// needed — before the next collide, before a reader, or before the Lagrangian points change — so
// every call sees exactly the reference's state.  The flux term q(u^t) the reference adds at the
// end of iteration t-1 is added by the collide of step t; iblb_get_flux() adds the not-yet-collided
// last term on demand.
//
// Slabs and ghost columns.  A context owns the columns [x_begin, x_begin + ncol) of the lattice.
// Every population buffer holds `gc` ghost columns on each side of them (columns -gc .. -1 and
// ncol .. ncol+gc-1 of the same interleaved layout, contiguous with the slab's own columns).  A
// slab of a group receives its neighbours' edge columns there — d whole columns per side, one
// contiguous block each way, sent and received by RCCL in place (no pack kernel, no slot map) —
// and every kernel reads them like its own columns.  `ghost` records how many of them hold the
// current state.  A lone slab wraps periodically inside the kernels and fills its ghosts (with
// its own edge columns) only for IB band trapezoids that cross x = 0.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <thread>
#include <vector>

#include "../../include/iblb.h"

#include "band_plan.h"
#include "cilia_kernels.h"
#include "iblb_kernels.h"

namespace iblbh {
using namespace iblb;

enum Phase { PH_EMPTY = 0, PH_BOOT = 1, PH_RUN = 2 };
enum IbState { IB_NONE = 0, IB_PENDING = 1, IB_READY = 2 };
enum Transport { TR_NONE = 0, TR_LOCAL = 1, TR_RCCL = 2 };
enum EvKind { EV_FUSED = 0, EV_IB = 1, EV_HALO = 2, EV_SWEEP = 3, EV_SWEEPK = 4 };

constexpr long GUARD = 512;  // elements in front of / behind every population buffer
constexpr int BAND_PIN_SLOTS = 4;

long env_long(const char* name, long dflt);
extern std::string g_create_error;

// Scratch device buffer freed at scope exit.
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// An observer's schedule: iblb_step stops at the iterations next, next + stride, ... and runs it there.
struct Periodic {
    int stride = 1;
    long long next = 0;   // the iteration after which it runs next
    long long count = 0;  // runs since it was set (the averages: or reset)
    void arm(long long t) { next = t + stride; }  // the first run `stride` iterations after t; count stays
    void advance() { next += stride; ++count; }
    void clear() { *this = Periodic{}; }
};

}  // namespace iblbh

struct iblb_ctx {
    iblb_config cfg{};
    int nx = 0, ny = 0, x_begin = 0, ncol = 0;
    int prec = IBLB_PREC_F64;
    size_t esize = 8;
    int V = 2, nch = 1;
    iblb::Layout L{};
    int gc = 0;       // ghost columns per side in every population buffer and in the dense force
    long fplane = 0;  // plane stride of the dense force and the boot fields: (ncol + 2 gc) * rows
    int device = 0;
    // kernel configuration: measured defaults; the IBLB_* knobs of INTEGRATION.md §4
    bool sweep_on = true;       // multi-iteration sweeps (IBLB_SWEEP)
    int sweep_w = 4, sweep_vs = 2;  // two-iteration sweeps: columns per wave, cells per lane
    int sweep_depth = 5;        // K iterations per deep launch (IBLB_SWEEP_DEPTH; 2 = two-step only)
    int deep_w = 128, deep_vs = 2, deep_balance = 1;  // IBLB_DEEP_W / _VS / _BALANCE
    iblb::DeepBuild deep_build{};  // the deep sweeps' build features (iblb_ctx.hip: the measured default; IBLB_DEEP_BUILD)
    int slab_vs = 1;            // cells per lane of a group slab's deep sweeps
    int reserved_cus = 0, ncu = 0;  // CUs kept free of the compute stream (RCCL groups), device CUs
    std::vector<uint32_t> comp_mask;  // the compute stream's CU mask when reserved_cus > 0
    hipStream_t stream = nullptr;
    iblb::Coef coef{};
    iblb::KConst kc{};  // collide constants folded from coef (kernel arguments)
    // populations: two buffers (ping-pong) in one allocation, each (ncol + 2 gc) columns; g[i]
    // points at column 0 of buffer i; `cur` holds the state
    char* g_alloc = nullptr;
    void* g[2] = {nullptr, nullptr};
    int cur = 0;
    long buf_elems = 0;  // elements of one buffer (ghost columns included)
    // boot arrays (slab layout, plane stride fplane)
    double* rho0 = nullptr;
    double* u0 = nullptr;
    double* force0 = nullptr;
    // immersed boundary
    int max_points = 0, ns = 0;
    bool cilia_on = false;  // on-device cilia kinematics (iblb_set_cilia)
    iblb_cilia cilia{};
    float* cil_samples = nullptr;  // the reference's d_boundary [5 * 9600 * c_num]
    float* cil_lasts = nullptr;    // [2 * 9600 * c_num]
    float* cil_bpoints = nullptr;  // [5 * 96 * c_num]
    float* d_s = nullptr;
    float* d_us = nullptr;
    float* d_Fs = nullptr;
    int* d_eps = nullptr;
    float* d_Fs_sum = nullptr;     // F_s summed over an RCCL group (reader scratch)
    std::vector<float> pts_host;   // (x, y) of the static points (band plans)
    // points given ahead (iblb_set_lagrangian_steps): entry i is used by iteration sch_t0 + i;
    // sch_cur is the entry of the current points (pts_*)
    float* d_sch_s = nullptr;
    float* d_sch_us = nullptr;
    int* d_sch_eps = nullptr;
    size_t sch_cap = 0;  // entries allocated
    int sch_n = 0, sch_cur = -1;
    long long sch_t0 = 0;
    std::vector<float> sch_x;       // [sch_n][ns][2]: (x, y) of every entry (band plans)
    std::vector<float> sch_x_prev;  // the points before the schedule (their force may be owed)
    bool cil_sched = false;         // the schedule is the cilia kinematics run ahead (cilia_schedule)
    // dense IB force [2][(ncol + 2 gc) * rows] and a flag per (column, row chunk); fdense and
    // flags point at column 0
    double* fd_alloc = nullptr;
    double* fdense = nullptr;
    uint8_t* fl_alloc = nullptr;
    uint8_t* flags = nullptr;
    // ---- IB band cycle (ctx_band.hip) ----
    int band_on = 1;             // IBLB_IB_BAND
    bool band_valid = false;     // the installed plan covers the points of the next cycle
    bool band_dirty = false;     // static points changed (or the context was linked): plan again
    iblbh::BandPlan plan;        // the installed plan (band_plan.h): assigned whole, and only with band_valid
    int* band_pin[iblbh::BAND_PIN_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    size_t band_pin_cap = 0;     // ints per slot
    hipEvent_t band_pin_ev[iblbh::BAND_PIN_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    int band_pin_i = 0, band_pin_cur = -1;
    int* band_tab = nullptr;     // the installed plan's level tables (a pinned slot)
    bool band_run = false;       // the last step was a band cycle on band_st / deep_st (not joined)
    long long band_retry_t = 0;  // a declined schedule plan: next attempt at this iteration
    long long band_hold_t = -1;  // the points were replaced (iblb_set_lagrangian, iblb_set_cilia) with the old points'
                                 // force^t in the dense buffer, outside any plan of the new points: iteration
                                 // band_hold_t is a one-step iteration (it consumes the force over the whole slab)
    hipEvent_t band_end = nullptr; // recorded on the deep stream at the end of the last band cycle
    char* s_alloc = nullptr;     // two scratch population buffers of the trapezoid (layout of g)
    void* sbuf[2] = {nullptr, nullptr};
    int band_merge = 1;          // IBLB_BAND_MERGE: 1 auto, 2 always, 0 never: each level's launch also
                                 // evaluates the next level's force (merged chain)
    int band_vhalf_env = 1;      // IBLB_BAND_VHALF: f32 chained chain's level launches at half-height waves
    double* bf_alloc = nullptr;  // merged chain: two more dense force buffers (levels j % 3 = 1, 2) ...
    uint8_t* bfl_alloc = nullptr;  // ... and their chunk flags, one per 64 * V rows.  Full-height levels clear a flag
                                   // with the force rows they consume; f32 half-height levels (plan.vhalf) leave
                                   // the flags set between cycles, here and in `flags`, since two waves read each:
                                   // there only the force rows are zeroed, and a set flag over zero rows is harmless
    double* bfd[2] = {nullptr, nullptr};
    uint8_t* bfl[2] = {nullptr, nullptr};
    int band_par_env = 1;        // IBLB_BAND_PAR: the last level beside the deep sweep (lone and group slabs)
    bool band_prev_par = false;  // the last band cycle ran it (its deep sweep ended on ev_deep)
    hipEvent_t ev_deep = nullptr;  // the last band cycle's deep sweep done (PAR cycles)
    int band_reserve = 0;        // CUs of the band chain's stream (0: one stream, in sequence; -2: unmasked)
    bool band_sticky = false;    // keep the streams while a schedule runs
    hipStream_t band_st = nullptr;  // the band chain (masked to the reserved CUs)
    hipStream_t deep_st = nullptr;  // the cycle's deep sweep (masked to the other CUs)
    hipEvent_t ev_b0 = nullptr, ev_bd = nullptr;
    // flux: d_Q[0] cumulative, d_Q[1] scratch
    double* d_Q = nullptr;
    // iblb_reduce_fields: device scratch (partials and result, ReduceGeom) and the host copy of the result;
    // both grow on demand and stay with the context
    double* red_buf = nullptr;
    size_t red_cap = 0;  // doubles allocated
    std::vector<double> red_host;
    // passive tracers (iblb_set_tracers): SoA positions in double, wraps in x counted in laps.  tr_n == 0:
    // none.  With tracers iblb_step stops at the iterations of tr_ev and updates them there (ctx_observe.hip)
    double* tr_x = nullptr;
    double* tr_y = nullptr;
    int* tr_laps = nullptr;
    long long tr_n = 0;
    iblbh::Periodic tr_ev;  // count: updates done since iblb_set_tracers
    // the tracers' motion model (iblb_set_tracer_model).  tr_status == nullptr: none, the plain update runs.
    // tr_status [tr_n] IBLB_TRACER_ALIVE / _AT_BOTTOM / _AT_TOP, tr_hit [tr_n] the hit iteration (-1 while alive),
    // tr_dep [2 ncol] the scratch of the per-column deposit counts (bottom, top), tr_amp = sqrt(6 D stride)
    int* tr_status = nullptr;
    long long* tr_hit = nullptr;
    unsigned long long* tr_dep = nullptr;
    iblb_tracer_model tr_model{};
    double tr_amp = 0.0;
    // time- and phase-averaged fields (iblb_set_average).  av_fields == 0: none.  With averaging iblb_step
    // stops at the iterations of av_ev and adds a sample to bin av_ev.count % av_nbins there.
    // av_buf: [av_nbins][av_planes][av_win.nx * av_win.ny] doubles, a plane in the order the accumulate
    // kernel's lanes run (y fastest); the planes of a bin: the sums of the set bits of av_fields in
    // ascending order, their squares' sums (IBLB_AVG_SQ), then ux*uy (IBLB_AVG_UXUY)
    double* av_buf = nullptr;
    iblb_window av_win{};
    unsigned av_fields = 0, av_flags = 0;
    int av_nbins = 1, av_planes = 0;
    iblbh::Periodic av_ev;  // count: samples taken since iblb_set_average / iblb_reset_average
    std::vector<long long> av_count;  // samples per bin
    // passive scalar (iblb_set_scalar).  sc_alloc == nullptr: none.  One allocation: two buffers of five planes
    // (sc_g, ping-pong; sc_cur holds the post-stream populations) and the two-plane velocity scratch sc_uv, each
    // plane ncol * L.rows doubles, [x * rows + y].  With a scalar iblb_step stops at the iterations of sc_ev and
    // does sc_ev.stride substeps there with the velocity of that moment (ctx_observe.hip)
    double* sc_alloc = nullptr;
    double* sc_g[2] = {nullptr, nullptr};
    double* sc_uv = nullptr;
    int sc_cur = 0;
    iblb_scalar sc_cfg{};   // as given (stride also in sc_ev)
    iblbh::Periodic sc_ev;  // count: events run since iblb_set_scalar
    // the scalar's source (iblb_set_scalar_source).  sc_src_present == 0: none.  sc_src_field: one plane in the
    // scalar's layout; sc_src_walls: [4 * ncol], wall_flux[0], wall_flux[1], wall_value[0], wall_value[1]; a NULL
    // array of the call is held as zeros (wall_value: as the uniform value).  Lives and dies with the scalar.
    double* sc_src_field = nullptr;
    double* sc_src_walls = nullptr;
    double sc_src_decay = 0.0;
    unsigned sc_src_present = 0;  // the `present` bits of iblb_scalar_source_info
    // the scalar's uptake (iblb_set_scalar_uptake).  sc_up_present == 0: none.  sc_up: one allocation of [6 * ncol],
    // a, total, last of ScalarUptake ([2 * ncol] each, wall 0 then wall 1); a NULL rate array of the call is held as
    // zeros in a.  Lives and dies with the scalar.
    double* sc_up = nullptr;
    unsigned sc_up_present = 0;   // the `present` bits of iblb_scalar_uptake_info
    long long sc_up_substeps = 0; // substeps accumulated since the set / the reset
    // the scalar's open ends in x (iblb_set_scalar_ends).  sc_end_present == 0: none, the scalar is periodic.  sc_end:
    // one allocation of [6 * ny], value, total, last of ScalarEnds ([2 * ny] each, the left end then the right one); a
    // NULL profile of the call is held as the uniform value.  Lives and dies with the scalar.
    double* sc_end = nullptr;
    int sc_end_kind[2] = {0, 0};
    double sc_end_value[2] = {0.0, 0.0};  // as given
    unsigned sc_end_present = 0;   // the `present` bits of iblb_scalar_ends_info
    long long sc_end_substeps = 0; // substeps accumulated since the set / the reset
    // the scalar's transport gauges (iblb_set_scalar_gauges).  sc_gau == nullptr: none.  sc_gau: one allocation, the
    // totals right, left ([n_stations * ny] each), up, down ([n_levels * ncol] each) and then the index arrays col
    // ([ncol]) and row ([ny]) of ScalarGauges.  Lives and dies with the scalar.
    double* sc_gau = nullptr;
    std::vector<int> sc_gau_station, sc_gau_level;  // as given
    long long sc_gau_substeps = 0; // substeps accumulated since the set / the reset
    // history recorder (iblb_set_history).  hi_n == 0: none.  With a history iblb_step stops at the iterations of
    // hi_ev and appends record hi_ev.count to slot hi_ev.count % hi_cap of the ring there.  hi_buf: one allocation,
    // the ring [hi_cap][hi_planes][hi_n] doubles, the statistics (eight arrays of hi_planes * hi_n 8-byte entries:
    // count, nonfinite, sum, sum_sq, min, max, min_rec, max_rec) and, for fixed probes, the positions x [hi_n] then
    // y [hi_n].  Under IBLB_HIST_TRACERS the positions are tr_x, tr_y, tr_laps and hi_n == tr_n
    double* hi_buf = nullptr;
    long long hi_n = 0, hi_cap = 0;
    unsigned hi_fields = 0, hi_flags = 0;
    int hi_planes = 0;
    iblbh::Periodic hi_ev;  // count: records taken since iblb_set_history / iblb_reset_history
    std::vector<long long> hi_iter;  // the iteration of the record in each slot
    // state machine
    int phase = iblbh::PH_EMPTY;
    long long t = 0;
    int ib_state = iblbh::IB_NONE;
    int ghost = 0;  // ghost columns per side holding the current state's neighbour columns
    int bnd_w = INT_MAX;  // edge columns per side the last step wrote on the comm stream
                          // (INT_MAX: the comm stream already follows the whole last step)
    // transport
    int transport = iblbh::TR_NONE;
    iblb_ctx* left = nullptr;
    iblb_ctx* right = nullptr;
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    bool self_ring = false;  // one rank that is its own neighbour over RCCL (IBLB_RCCL_SELF, rehearsal)
    std::vector<int> slab_begin, slab_count;  // every rank's columns (RCCL group)
    int min_slab = 0;                         // the narrowest slab of the group
    hipStream_t comm_stream = nullptr;  // RCCL halo exchange and boundary columns, beside the interior
    hipStream_t rccl_last = nullptr;    // the stream of the last RCCL call (ops stay in issue order)
    hipEvent_t ev_bnd = nullptr;  // comm-stream work of the last step done
    hipEvent_t ev_int = nullptr;  // compute-stream work of the last step done
    hipEvent_t ev_int2 = nullptr; // spare: a deep slab cycle's interior signals it on completion
    hipEvent_t ev_pre = nullptr;  // compute-stream work before this step
    hipEvent_t ev_x = nullptr;    // the band cycle's halo exchange done
    hipEvent_t ev_rccl = nullptr; // orders RCCL calls across streams
    bool deep_chain = false;      // the last compute work is a deep slab cycle's (interior first) ...
    long long deep_chain_t = -1;  // ... that ended at this t with this cur: ev_int follows its interior
    int deep_chain_cur = -1;
    bool overlap = true;          // IBLB_OVERLAP
    // deep slab cycles: the interior's edge waves wait on a device word the comm stream's boundary
    // sweeps signal (IBLB_EDGE_FLAG, default on) instead of the compute queue waiting for ev_bnd
    int edge_flag = 1;  // 1: two-way device handshake, 2: one way (interior waits only), 0: queue waits
    unsigned* sig = nullptr;      // device words: [0] sequence number of the last boundary launch done,
                                  // [16] edge waves of the slab interiors done (ctx_step.hip:deep_slab_step),
                                  // [24] band cycles whose exchange landed (ctx_band.hip:band_step)
    unsigned sig_n = 0;           // boundary launches signalled so far (the value of the last one)
    unsigned done_n = 0;          // interior edge waves launched so far (the done word's value once they end)
    unsigned bx_n = 0;            // band cycles whose exchange the level-0 IB signalled in sig[24] (ctx_band.hip)
    bool bx_dev = false;          // this band cycle's boundary sweeps wait on sig[24] (set by band_step)
    bool bnd_in_end = false;      // the last band cycle's band_end follows its boundary sweeps (ev_bnd)
    bool int_unrec = false;       // the last interior carried no event: ev_int is recorded on demand
    unsigned* sig_err = nullptr;  // host-coherent word: an edge wave's bounded wait timed out
    // the device waits' bound (IBLB_WAIT_TIMEOUT_S / iblb_set_wait_timeout, default 600 s): wall-clock
    // time, in ticks of the device's constant clock (hipDeviceAttributeWallClockRate)
    double wait_timeout_s = 600.;
    double clock_hz = 0.;  // the device wall clock's rate
    unsigned long long wait_ticks = 0;
    long long dev_wait_launches = 0;  // launches whose waves waited on a device word (iblb_timing)
    // the last deep launch's build: MODE, VS, waves per SIMD, VGPRs (iblb_timing), and its collide's force
    // build (iblb_deep_force_build: 1 x-only, 0 general, -1 no deep launch yet)
    int deep_kinfo[5] = {0, 0, 0, 0, -1};
    // test hold (IBLB_TEST_HOLD=<n>:<ms>): exchange number n since the attach (0-based) starts after a
    // one-wave kernel that a host thread releases ms milliseconds after its submission, as if a
    // neighbour rank reached that exchange late (tests/test_gpu_wait.py)
    long long hold_x = -1, n_exch = 0;
    int hold_ms = 0;
    unsigned* hold_word = nullptr;  // host-coherent
    std::thread hold_thread;
    // profiling
    int prof = 0;  // 1: events around every launch; 2: the deep launches' own signals only (iblb_set_profiling)
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    double fused_ms = 0., ib_ms = 0., halo_ms = 0., sweep_ms = 0., sweepk_ms = 0.;
    long long fused_launches = 0, fused_cells = 0, sweep_launches = 0, sweep_cells = 0, sweepk_launches = 0,
              sweepk_cells = 0;
    long long band_cycles = 0, band_merged_cycles = 0, band_par_cycles = 0;  // IB band cycles run (counted without events too)
    long long deep_launches = 0, deep_iterations = 0;  // deep launches and the iterations they advanced (no events needed)
    bool band_own_build = false;  // the band cycle's deep sweep in the configured (not the chain-friendly) build
    struct EvRec { int kind; size_t idx; long long cells; };
    std::vector<EvRec> ev_kind;
    std::string err;
};

namespace iblbh {

int fail(iblb_ctx* c, int code, const std::string& msg);
int hip_fail(iblb_ctx* c, hipError_t e, const char* what);

#define HIP_TRY(c, expr)                                               \
    do {                                                               \
        hipError_t e_ = (expr);                                        \
        if (e_ != hipSuccess) return ::iblbh::hip_fail((c), e_, #expr); \
    } while (0)

#define NCCL_TRY(c, expr)                                                                                      \
    do {                                                                                                       \
        ncclResult_t r_ = (expr);                                                                              \
        if (r_ != ncclSuccess)                                                                                 \
            return ::iblbh::fail((c), IBLB_ERR_COMM, std::string(#expr) + ": " + ncclGetErrorString(r_));       \
    } while (0)

template <typename T>
inline T* gptr(iblb_ctx* c, int which) { return (T*)c->g[which]; }

inline bool single_slab(const iblb_ctx* c) {
    return c->ncol == c->nx && c->transport != TR_LOCAL && c->nranks <= 1 && !c->self_ring;
}
inline bool rccl_multi(const iblb_ctx* c) { return c->transport == TR_RCCL && (c->nranks > 1 || c->self_ring); }
inline bool ib_active(const iblb_ctx* c) { return c->max_points > 0 && c->ns > 0; }
inline bool is_f64(const iblb_ctx* c) { return c->prec == IBLB_PREC_F64; }

// schedule entry of iteration it (clamped to the last one)
inline int sched_entry(const iblb_ctx* c, long long it) {
    const long long e = it - c->sch_t0;
    return (int)std::max(0LL, std::min(e, (long long)c->sch_n - 1));
}
template <typename P>
inline P* sched_ptr(P* base, const iblb_ctx* c, int e, int per_point) { return base + (size_t)e * per_point * c->ns; }
// the current points become those of schedule entry e (no copy: launches and readers take pts_*)
inline void sched_use(iblb_ctx* c, int e) {
    if (c->sch_n > 0) c->sch_cur = e;
}
// arrays of the current points: the schedule entry in use, else the static points
inline const float* pts_s(const iblb_ctx* c) {
    return c->sch_n > 0 && c->sch_cur >= 0 ? sched_ptr(c->d_sch_s, c, c->sch_cur, 2) : c->d_s;
}
inline const float* pts_us(const iblb_ctx* c) {
    return c->sch_n > 0 && c->sch_cur >= 0 ? sched_ptr(c->d_sch_us, c, c->sch_cur, 2) : c->d_us;
}
inline const int* pts_eps(const iblb_ctx* c) {
    return c->sch_n > 0 && c->sch_cur >= 0 ? sched_ptr(c->d_sch_eps, c, c->sch_cur, 1) : c->d_eps;
}
// the points of iteration it (a schedule entry, or the static points)
inline void pts_of(const iblb_ctx* c, long long it, const float** s, const float** us, const int** e) {
    if (c->sch_n > 0) {
        const int k = sched_entry(c, it);
        *s = sched_ptr(c->d_sch_s, c, k, 2);
        *us = sched_ptr(c->d_sch_us, c, k, 2);
        *e = sched_ptr(c->d_sch_eps, c, k, 1);
    } else {
        *s = c->d_s;
        *us = c->d_us;
        *e = c->d_eps;
    }
}

// periodic images of a lone slab: the edge columns of buffer g itself
template <typename T>
Halo<T> halo_at(const iblb_ctx* c, const T* g) {
    Halo<T> H;
    for (int p = 0; p < 3; ++p) {
        H.left[p] = g + left_plane(p) * c->L.plane + (long)(c->L.ncol - 1) * c->L.col;
        H.right[p] = g + right_plane(p) * c->L.plane;
    }
    return H;
}
// ghost columns -1 and ncol of buffer g
template <typename T>
Halo<T> ghost_halo(const iblb_ctx* c, const T* g) {
    Halo<T> H;
    for (int p = 0; p < 3; ++p) {
        H.left[p] = g + left_plane(p) * c->L.plane - c->L.col;
        H.right[p] = g + right_plane(p) * c->L.plane + (long)c->L.ncol * c->L.col;
    }
    return H;
}
template <typename T>
Halo<T> halo_of(iblb_ctx* c, int which) {
    const T* g = gptr<T>(c, which);
    return single_slab(c) ? halo_at<T>(c, g) : ghost_halo<T>(c, g);
}

// ---- profiling (iblb_ctx.hip) ----
int ev_begin(iblb_ctx* c, size_t* idx, hipStream_t st = nullptr);
int ev_end(iblb_ctx* c, size_t idx, int kind, long long cells = 0, hipStream_t st = nullptr);
// timing events that a launch carries itself (hipExtLaunchKernelGGL start / stop: the kernel's own
// dispatch and completion signals, no marker packets); null when not profiling
int ev_kernel(iblb_ctx* c, size_t* idx, hipEvent_t* start, hipEvent_t* stop);
int ev_kernel_end(iblb_ctx* c, size_t idx, int kind, long long cells);

// ---- halo / force (ctx_step.hip) ----
int rccl_order(iblb_ctx* c, hipStream_t st);
int join_comm(iblb_ctx* c);
int exchange(iblb_ctx* c, hipStream_t st, int d);
int fill_ghosts_periodic(iblb_ctx* c, int which, int d, hipStream_t st);
int ensure_halo(iblb_ctx* c);
int ensure_force(iblb_ctx* c);
int ib_ghost(iblb_ctx* c, const void* g, int gc, int clo, int chi, const float* s, const float* us, const int* eps,
             int part, hipStream_t st, unsigned* sig = nullptr, unsigned sig_val = 0, int wlo = 0, int whi = 0);
int check_ready(iblb_ctx* c);
int check_wait_err(iblb_ctx* c);  // after a synchronize: did an edge wave's wait time out?
int set_wait_ticks(iblb_ctx* c);  // wait_ticks from wait_timeout_s and the device's wall-clock rate
int hold_release(iblb_ctx* c);    // join the test hold's host thread (IBLB_TEST_HOLD)
int prepare_read(iblb_ctx* c);
int free_boot(iblb_ctx* c);
int alloc_zero(iblb_ctx* c, void** p, size_t bytes);
int run_cilia(iblb_ctx* c);
template <typename T>
Sweep2Args<T> sweep_args(iblb_ctx* c, int col_begin, int col_step, int col_end, int nsweep, int W);

// ---- band cycle (ctx_band.hip) ----
bool band_ready(const iblb_ctx* c);
int band_step_any(iblb_ctx* c);
int plan_bands(iblb_ctx* c, const std::vector<float>& xy);
int plan_cycle(iblb_ctx* c);
int band_join(iblb_ctx* c);     // the context's stream after a run of band cycles
int retire_points(iblb_ctx* c);  // owed force evaluated; an active schedule entry becomes the static points
int cilia_schedule(iblb_ctx* c, int n);  // cilia kinematics of the next n iterations as a schedule
int cilia_schedule_end(iblb_ctx* c);
bool band_possible(const iblb_ctx* c);  // the band cycle may run on this context (points aside)
int band_release(iblb_ctx* c);  // streams, events, pinned tables, scratch buffers

// ---- readers (ctx_read.hip) ----
// the window (NULL: the whole lattice) checked, and this slab's samples [*i_first, *i_first + *nxl) of it
int window_part(iblb_ctx* c, const iblb_window* w, iblb_window* win, int* i_first, int* nxl);
// the windowed kernels' arguments for samples [lo, lo + nxl) of win; point_args: their state-dependent part (no window)
FieldsArgs window_args(iblb_ctx* c, const iblb_window& win, int lo, int nxl, unsigned fields);
inline FieldsArgs point_args(iblb_ctx* c, unsigned fields) { return window_args(c, {0, 0, 1, 1, 1, 1}, 0, 1, fields); }
int check_positions(iblb_ctx* c, long long n, const double* x, const double* y);
int group_refused(iblb_ctx* c, const char* what);

// ---- observers (ctx_observe.hip): run by iblb_step on the context's stream, no host synchronise ----
long long next_event(const iblb_ctx* c);  // the next iteration at which an observer runs (LLONG_MAX: none set)
int run_events(iblb_ctx* c);              // every observer due at c->t: the scalar, the tracers, the averages, the history
void tracers_free(iblb_ctx* c);
void history_free(iblb_ctx* c);
void average_free(iblb_ctx* c);
void scalar_free(iblb_ctx* c);

// ---- observers in checkpoints (ctx_observe.hip; the sections' payloads are laid out above the checkpoint code
// of iblb_ctx.hip).  kind: iblbck::K_SCALAR, K_TRACERS, K_AVERAGE (ckpt_format.h) ----
// A section's payload parsed and checked on the host: everything its observer needs to go on
struct CkScalar {
    iblb_scalar cfg{};
    long long t0 = 0, events = 0;
    unsigned parts = 0;  // 1 source, 2 uptake, 4 ends, 8 gauges
    std::vector<double> pops;  // iblb_get_scalar_populations
    unsigned src_present = 0;
    double src_decay = 0.0;
    std::vector<double> src_field, src_walls;  // iblb_get_scalar_source; sc_src_walls
    unsigned up_present = 0;
    long long up_substeps = 0;
    std::vector<double> up;  // sc_up
    int end_kind[2] = {0, 0};
    double end_value[2] = {0.0, 0.0};
    unsigned end_present = 0;
    long long end_substeps = 0;
    std::vector<double> end;  // sc_end
    std::vector<int> station, level;
    long long gau_substeps = 0;
    std::vector<double> gau;  // the four totals of sc_gau
};
struct CkTracers {
    long long n = 0, t0 = 0, updates = 0;
    int stride = 1;
    std::vector<double> x, y;
    std::vector<int> laps;
};
struct CkAverage {
    iblb_window win{};
    unsigned fields = 0, flags = 0;
    int stride = 1, nbins = 1, planes = 0;
    long long t0 = 0, samples = 0;
    std::vector<long long> count;
    std::vector<double> bins;  // [nbins][planes][win.ny][win.nx]: every bin as iblb_get_average returns it
};
struct CkObservers {
    bool has[3] = {false, false, false};
    CkScalar sc;
    CkTracers tr;
    CkAverage av;
};
bool observer_set(const iblb_ctx* c, int kind);
// the payload of a set observer's section, read from the device (the streams synchronised by the caller)
int observer_pack(iblb_ctx* c, int kind, std::vector<char>* out);
// payload[k] of the sections has[k] of a file saved at iteration t, parsed into *o and checked against the context;
// changes nothing in the context (but its error text); empties the payloads it has parsed
int observers_parse(iblb_ctx* c, long long t, std::vector<char> payload[3], const bool has[3], CkObservers* o);
// the three observers removed, then those of o set as they were saved; c->t is the file's iteration.  On a failure
// all three are removed
int observers_restore(iblb_ctx* c, const CkObservers& o);

// ---- the read scaffold: what every reader and observer is made of ----
// f(g, H): the populations and the halo of the current state, typed by the context's precision; the
// launchers deduce their T from them.  Returns f's hipError_t.
template <typename F>
inline hipError_t with_state(iblb_ctx* c, F&& f) {
    if (is_f64(c)) return f(gptr<double>(c, c->cur), halo_of<double>(c, c->cur));
    return f(gptr<float>(c, c->cur), halo_of<float>(c, c->cur));
}

// the dense IB force of the current state (null: none evaluated, the body force alone)
inline const double* ib_force(const iblb_ctx* c) { return c->ib_state == IB_READY ? c->fdense : nullptr; }

constexpr unsigned IBLB_FIELD_ALL = IBLB_FIELD_RHO | IBLB_FIELD_UX | IBLB_FIELD_UY | IBLB_FIELD_VORT | IBLB_FIELD_SXX |
                                    IBLB_FIELD_SXY | IBLB_FIELD_SYY;
constexpr unsigned IBLB_QTY_ALL = IBLB_QTY_MOMX | IBLB_QTY_MOMY | IBLB_QTY_KE | IBLB_QTY_USQ;

constexpr unsigned IBLB_FIELD_SCALAR = IBLB_FIELD_C | IBLB_FIELD_CUX | IBLB_FIELD_CUY;  // FIELD_SCALAR_BITS

// at least one bit and none outside `known`: the fields every reader takes, or with IBLB_QTY_ALL what
// iblb_reduce_fields takes
inline int check_fields(iblb_ctx* c, unsigned fields, unsigned known = IBLB_FIELD_ALL | IBLB_FIELD_SCALAR) {
    if (fields != 0 && !(fields & ~known)) return IBLB_OK;
    return fail(c, IBLB_ERR_ARG, known & IBLB_QTY_ALL ? "fields: no quantity or an unknown IBLB_FIELD_* / IBLB_QTY_* bit"
                                                      : "fields: no field or an unknown IBLB_FIELD_* bit");
}

inline int check_vorticity(iblb_ctx* c, unsigned fields) {
    if (!(fields & IBLB_FIELD_VORT) || single_slab(c)) return IBLB_OK;
    return fail(c, IBLB_ERR_UNSUPPORTED,
                "vorticity needs the neighbour slabs' velocity and force: a lone slab only (compute it from "
                "the gathered u)");
}

// A scalar's field needs a scalar, which only a lone slab can hold.  Comes after every argument check and
// check_vorticity, before anything collective.
inline int check_scalar_fields(iblb_ctx* c, unsigned fields) {
    if (!(fields & IBLB_FIELD_SCALAR) || (c->sc_alloc && single_slab(c))) return IBLB_OK;
    return fail(c, IBLB_ERR_STATE,
                single_slab(c) ? "IBLB_FIELD_C / _CUX / _CUY: no scalar is set (iblb_set_scalar)"
                               : "IBLB_FIELD_C / _CUX / _CUY: a slab of a group holds no scalar");
}

// n values summed over the slabs of an RCCL group, on the context's stream; a lone slab: nothing
inline int group_sum(iblb_ctx* c, const void* send, void* recv, size_t n, ncclDataType_t type) {
    if (!rccl_multi(c)) return IBLB_OK;
    int rc = rccl_order(c, c->stream);
    if (rc) return rc;
    NCCL_TRY(c, ncclAllReduce(send, recv, n, type, ncclSum, c->comm, c->stream));
    return IBLB_OK;
}

// The end of a read: the context's stream synchronised, then blocking copies to the host.  Null
// destinations and empty copies are skipped (the synchronise is not).
struct HostCopy {
    void* host;
    const void* dev;
    size_t bytes;
};
inline int read_back(iblb_ctx* c, std::initializer_list<HostCopy> copies) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (const HostCopy& k : copies)
        if (k.host && k.bytes) HIP_TRY(c, hipMemcpy(k.host, k.dev, k.bytes, hipMemcpyDeviceToHost));
    return IBLB_OK;
}
inline int read_back(iblb_ctx* c, void* host, const void* dev, size_t bytes) {
    return read_back(c, {{host, dev, bytes}});
}

}  // namespace iblbh
