// ctx_observe.hip — the observers of a context (ctx.h): what iblb_step runs between the pieces of a call
// with the state held fixed.  Passive tracers (iblb_set_tracers), time- and phase-averaged fields
// (iblb_set_average), the passive scalar (iblb_set_scalar) and the history recorder (iblb_set_history: probe
// time series and tracer pathlines in a ring on the device), each on a Periodic schedule; iblb_step asks
// next_event where to cut a call and run_events to run what is due there.  Built from the read scaffold of
// ctx.h like the readers.  At the end: the observers' sections of a checkpoint, written from and restored into the
// context (iblb_save_checkpoint_ex, iblb_load_checkpoint in iblb_ctx.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ckpt_format.h"
#include "ctx.h"

namespace iblbh {

static void scalar_source_free(iblb_ctx* c) {
    for (void* p : {(void*)c->sc_src_field, (void*)c->sc_src_walls})
        if (p) (void)hipFree(p);
    c->sc_src_field = c->sc_src_walls = nullptr;
    c->sc_src_decay = 0.0;
    c->sc_src_present = 0;
}

static void scalar_uptake_free(iblb_ctx* c) {
    if (c->sc_up) (void)hipFree(c->sc_up);
    c->sc_up = nullptr;
    c->sc_up_present = 0;
    c->sc_up_substeps = 0;
}

static void scalar_ends_free(iblb_ctx* c) {
    if (c->sc_end) (void)hipFree(c->sc_end);
    c->sc_end = nullptr;
    c->sc_end_kind[0] = c->sc_end_kind[1] = 0;
    c->sc_end_value[0] = c->sc_end_value[1] = 0.0;
    c->sc_end_present = 0;
    c->sc_end_substeps = 0;
}

static void scalar_gauges_free(iblb_ctx* c) {
    if (c->sc_gau) (void)hipFree(c->sc_gau);
    c->sc_gau = nullptr;
    c->sc_gau_station.clear();
    c->sc_gau_level.clear();
    c->sc_gau_substeps = 0;
}

void scalar_free(iblb_ctx* c) {
    scalar_source_free(c);  // the source belongs to the scalar it was set on
    scalar_uptake_free(c);  // and so does the uptake
    scalar_ends_free(c);    // and the open ends
    scalar_gauges_free(c);  // and the gauges
    if (c->sc_alloc) (void)hipFree(c->sc_alloc);
    c->sc_alloc = c->sc_g[0] = c->sc_g[1] = c->sc_uv = nullptr;
    c->sc_cur = 0;
    c->sc_cfg = iblb_scalar{};
    c->sc_ev.clear();
}

static ScalarGeom scalar_geom(const iblb_ctx* c) {
    return ScalarGeom{c->ncol, c->ny, c->L.rows, (long)c->ncol * c->L.rows};
}

static ScalarRule scalar_rule(const iblb_scalar& k) {
    return ScalarRule{1.0 / k.tau, {k.wall_kind[0], k.wall_kind[1]}, {k.wall_value[0], k.wall_value[1]}};
}

// nullptr members without a source: the launchers then run the builds without one
static ScalarSource scalar_source(const iblb_ctx* c) {
    return ScalarSource{c->sc_src_field, c->sc_src_walls, c->sc_src_decay};
}

// nullptr members without an uptake: the launchers then run the builds without one
static ScalarUptake scalar_uptake(const iblb_ctx* c) {
    if (!c->sc_up) return ScalarUptake{nullptr, nullptr, nullptr};
    const size_t n = 2 * (size_t)c->ncol;
    return ScalarUptake{c->sc_up, c->sc_up + n, c->sc_up + 2 * n};
}

// nullptr members without open ends: the launchers then run the builds without them
static ScalarEnds scalar_ends(const iblb_ctx* c) {
    if (!c->sc_end) return ScalarEnds{{0, 0}, nullptr, nullptr, nullptr};
    const size_t n = 2 * (size_t)c->ny;
    return ScalarEnds{{c->sc_end_kind[0], c->sc_end_kind[1]}, c->sc_end, c->sc_end + n, c->sc_end + 2 * n};
}

// the doubles of the gauges' four totals: right, left ([n_stations * ny] each), up, down ([n_levels * ncol] each)
static size_t scalar_gauges_totals(const iblb_ctx* c) {
    return 2 * (c->sc_gau_station.size() * (size_t)c->ny + c->sc_gau_level.size() * (size_t)c->ncol);
}

// nullptr members without gauges: the launchers then run the builds without them
static ScalarGauges scalar_gauges(const iblb_ctx* c) {
    if (!c->sc_gau) return ScalarGauges{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t ns = c->sc_gau_station.size() * (size_t)c->ny, nl = c->sc_gau_level.size() * (size_t)c->ncol;
    double* t = c->sc_gau;
    const int2* idx = (const int2*)(t + 2 * (ns + nl));
    return ScalarGauges{idx, idx + c->ncol, t, t + ns, t + 2 * ns, t + 2 * ns + nl};
}

// the tracers' motion model (iblb_set_tracer_model): the tracers then take the plain update again
static void tracer_model_free(iblb_ctx* c) {
    for (void* p : {(void*)c->tr_status, (void*)c->tr_hit, (void*)c->tr_dep})
        if (p) (void)hipFree(p);
    c->tr_status = nullptr;
    c->tr_hit = nullptr;
    c->tr_dep = nullptr;
    c->tr_model = iblb_tracer_model{};
    c->tr_amp = 0.0;
}

void tracers_free(iblb_ctx* c) {
    tracer_model_free(c);  // the model belongs to the tracer set it was put on
    for (void* p : {(void*)c->tr_x, (void*)c->tr_y, (void*)c->tr_laps})
        if (p) (void)hipFree(p);
    c->tr_x = c->tr_y = nullptr;
    c->tr_laps = nullptr;
    c->tr_n = 0;
    c->tr_ev.clear();
}

void average_free(iblb_ctx* c) {
    if (c->av_buf) (void)hipFree(c->av_buf);
    c->av_buf = nullptr;
    c->av_win = iblb_window{};
    c->av_fields = c->av_flags = 0;
    c->av_nbins = 1;
    c->av_planes = 0;
    c->av_ev.clear();
    c->av_count.clear();
}

void history_free(iblb_ctx* c) {
    if (c->hi_buf) (void)hipFree(c->hi_buf);
    c->hi_buf = nullptr;
    c->hi_n = c->hi_cap = 0;
    c->hi_fields = c->hi_flags = 0;
    c->hi_planes = 0;
    c->hi_ev.clear();
    c->hi_iter.clear();
}

// the parts of hi_buf (ctx.h): entries of one plane set, doubles of one record, and the parts' places
static size_t history_entries(const iblb_ctx* c) { return (size_t)c->hi_planes * (size_t)c->hi_n; }
static double* history_stats_base(const iblb_ctx* c) { return c->hi_buf + (size_t)c->hi_cap * history_entries(c); }
static HistoryStats history_stats(const iblb_ctx* c) {
    const size_t e = history_entries(c);
    double* b = history_stats_base(c);
    return HistoryStats{(long long*)b,   (long long*)(b + e),     b + 2 * e, b + 3 * e, b + 4 * e,
                        b + 5 * e,       (long long*)(b + 6 * e), (long long*)(b + 7 * e)};
}
static const double* history_xy(const iblb_ctx* c) { return history_stats_base(c) + 8 * history_entries(c); }

// the statistics with nothing seen, for e entries: zeros, min = +inf, max = -inf, the record numbers -1
static std::vector<double> history_stats_blank(size_t e) {
    std::vector<double> h(8 * e, 0.0);
    std::fill_n(h.begin() + 4 * e, e, HUGE_VAL);
    std::fill_n(h.begin() + 5 * e, e, -HUGE_VAL);
    const long long none = -1;
    for (size_t j = 6 * e; j < 8 * e; ++j) std::memcpy(&h[j], &none, sizeof none);
    return h;
}

static size_t average_bin_elems(const iblb_ctx* c) {
    return (size_t)c->av_planes * (size_t)c->av_win.nx * (size_t)c->av_win.ny;
}

// One update of the tracers from the current state, on the context's stream: the state prepared as
// for a reader (the band streams joined, the owed IB force evaluated), then one launch: the plain kernel, or with
// a motion model (iblb_set_tracer_model) the particles'.
static int tracer_update(iblb_ctx* c) {
    int rc = band_join(c);
    if (rc || (rc = prepare_read(c))) return rc;
    const FieldsArgs a = point_args(c, IBLB_FIELD_UX | IBLB_FIELD_UY);
    const iblb_tracer_model& k = c->tr_model;
    const ParticleStep P{{k.drift[0], k.drift[1]}, c->tr_amp, {k.wall[0], k.wall[1]}, k.seed, c->tr_ev.count, c->t};
    HIP_TRY(c, with_state(c, [&](auto* g, auto H) {
        if (c->tr_status)
            return launch_particle_advect(g, c->L, H, a, (long)c->tr_n, c->tr_ev.stride, P, c->tr_x, c->tr_y, c->tr_laps,
                                          c->tr_status, c->tr_hit, c->stream);
        return launch_tracer_advect(g, c->L, H, a, (long)c->tr_n, c->tr_ev.stride, c->tr_x, c->tr_y, c->tr_laps, c->stream);
    }));
    c->tr_ev.advance();
    return IBLB_OK;
}

// One sample of the averaged fields from the current state, on the context's stream: the state prepared
// as for a reader (the band streams joined, the owed IB force evaluated), then one launch.
static int average_update(iblb_ctx* c) {
    if (!single_slab(c))  // the context joined a group after iblb_set_average: its window is the whole lattice's
        return fail(c, IBLB_ERR_UNSUPPORTED, "averaging: a lone slab only; remove it before joining a group");
    int rc = check_scalar_fields(c, c->av_fields);  // (iblb_set_scalar keeps the scalar under such an average)
    if (rc) return rc;
    rc = band_join(c);
    if (rc || (rc = prepare_read(c))) return rc;
    const int bin = (int)(c->av_ev.count % c->av_nbins);
    const FieldsArgs a = window_args(c, c->av_win, 0, c->av_win.nx, c->av_fields);
    double* acc = c->av_buf + (size_t)bin * average_bin_elems(c);
    HIP_TRY(c, with_state(c, [&](auto* g, auto H) {
        return launch_average_accum(g, c->L, H, a, c->av_flags, acc, c->stream);
    }));
    c->av_ev.advance();
    c->av_count[bin]++;
    return IBLB_OK;
}

// One event of the scalar on the context's stream: the state prepared as for a reader (the band streams
// joined, the owed IB force evaluated), then `stride` substeps with the velocity of this state: the first
// evaluates it from the fluid populations and leaves it in the scratch, the others read the scratch.  With a source
// (iblb_set_scalar_source) every substep runs the SOURCE build, without one the build that has none; likewise the
// UPTAKE builds with an uptake (iblb_set_scalar_uptake), whose accumulators then take every substep of the event, and
// the ENDS builds with open ends (iblb_set_scalar_ends) and the GAUGES builds with gauges (iblb_set_scalar_gauges).
static int scalar_update(iblb_ctx* c) {
    if (!single_slab(c))  // the context joined a group after iblb_set_scalar: its lattice is the whole lattice's
        return fail(c, IBLB_ERR_UNSUPPORTED, "scalar: a lone slab only; remove it before joining a group");
    int rc = band_join(c);
    if (rc || (rc = prepare_read(c))) return rc;
    const FieldsArgs a = point_args(c, IBLB_FIELD_UX | IBLB_FIELD_UY);
    const ScalarGeom S = scalar_geom(c);
    const ScalarRule R = scalar_rule(c->sc_cfg);
    const ScalarSource Q = scalar_source(c);
    const ScalarUptake U = scalar_uptake(c);
    const ScalarEnds E = scalar_ends(c);
    const ScalarGauges G = scalar_gauges(c);
    HIP_TRY(c, with_state(c, [&](auto* g, auto H) {
        return launch_scalar_first(g, c->L, H, a, S, R, Q, U, E, G, c->sc_g[c->sc_cur], c->sc_g[c->sc_cur ^ 1], c->sc_uv,
                                   c->stream);
    }));
    c->sc_cur ^= 1;
    for (int k = 1; k < c->sc_ev.stride; ++k) {
        HIP_TRY(c, launch_scalar_next(S, R, Q, U, E, G, c->sc_g[c->sc_cur], c->sc_g[c->sc_cur ^ 1], c->sc_uv, c->stream));
        c->sc_cur ^= 1;
    }
    c->sc_ev.advance();
    if (c->sc_up) c->sc_up_substeps += c->sc_ev.stride;
    if (c->sc_end) c->sc_end_substeps += c->sc_ev.stride;
    if (c->sc_gau) c->sc_gau_substeps += c->sc_ev.stride;
    return IBLB_OK;
}

// One record of the history from the current state, on the context's stream: the state prepared as for a
// reader (the band streams joined, the owed IB force evaluated), then one launch that writes the record into
// its slot of the ring and folds it into the statistics.  The slot's iteration is kept on the host.
static int history_update(iblb_ctx* c) {
    if (!single_slab(c))  // the context joined a group after iblb_set_history: its probes are the whole lattice's
        return fail(c, IBLB_ERR_UNSUPPORTED, "history: a lone slab only; remove it before joining a group");
    int rc = check_scalar_fields(c, c->hi_fields);  // (iblb_set_scalar keeps the scalar under such a history)
    if (rc) return rc;
    const bool follow = (c->hi_flags & IBLB_HIST_TRACERS) != 0;
    if (follow && c->tr_n != c->hi_n)  // (iblb_set_tracers keeps the tracers under such a history)
        return fail(c, IBLB_ERR_STATE, "history: the tracers it follows are gone");
    rc = band_join(c);
    if (rc || (rc = prepare_read(c))) return rc;
    const long long m = c->hi_ev.count;
    const size_t slot = (size_t)(m % c->hi_cap);
    const FieldsArgs a = point_args(c, c->hi_fields);
    const double* x = follow ? c->tr_x : history_xy(c);
    const double* y = follow ? c->tr_y : history_xy(c) + c->hi_n;
    const int* laps = follow ? c->tr_laps : nullptr;
    double* rec = c->hi_buf + slot * history_entries(c);
    const HistoryStats st = history_stats(c);
    HIP_TRY(c, with_state(c, [&](auto* g, auto H) {
        return launch_history_record(g, c->L, H, a, (long)c->hi_n, x, y, laps, m, rec, st, c->stream);
    }));
    c->hi_iter[slot] = c->t;
    c->hi_ev.advance();
    return IBLB_OK;
}

long long next_event(const iblb_ctx* c) {
    long long next = LLONG_MAX;
    if (c->tr_n > 0) next = std::min(next, c->tr_ev.next);
    if (c->av_fields) next = std::min(next, c->av_ev.next);
    if (c->sc_alloc) next = std::min(next, c->sc_ev.next);
    if (c->hi_n > 0) next = std::min(next, c->hi_ev.next);
    return next;
}

// No observer changes the fluid state, but an average may sample the scalar: the scalar's event runs first, so
// that a sample at a common iteration sees C after that iteration's event (include/iblb.h).  The history runs
// last: a pathline record holds the tracers after that iteration's update
int run_events(iblb_ctx* c) {
    int rc = IBLB_OK;
    if (c->sc_alloc && c->t == c->sc_ev.next && (rc = scalar_update(c))) return rc;
    if (c->tr_n > 0 && c->t == c->tr_ev.next && (rc = tracer_update(c))) return rc;
    if (c->av_fields && c->t == c->av_ev.next && (rc = average_update(c))) return rc;
    if (c->hi_n > 0 && c->t == c->hi_ev.next) rc = history_update(c);
    return rc;
}

}  // namespace iblbh

using namespace iblbh;

extern "C" {

// ---- passive tracers ----------------------------------------------------------------------------------
int iblb_set_tracers(iblb_ctx* c, long long n, const double* x, const double* y, int stride) {
    if (!c) return IBLB_ERR_ARG;
    if (n < 0) return fail(c, IBLB_ERR_ARG, "n is negative");
    if (stride < 1) return fail(c, IBLB_ERR_ARG, "stride must be >= 1");
    if (n > 0 && (!x || !y)) return fail(c, IBLB_ERR_ARG, "x or y is NULL");
    if (c->hi_n > 0 && (c->hi_flags & IBLB_HIST_TRACERS))
        return fail(c, IBLB_ERR_STATE, "iblb_set_tracers: the current history follows the tracers; remove the history first");
    if (!single_slab(c)) return group_refused(c, "iblb_set_tracers");
    int rc = check_positions(c, n, x, y);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (n == 0) {
        tracers_free(c);
        return IBLB_OK;
    }
    // the new arrays first: a failed allocation leaves the previous tracers as they were
    const size_t np = (size_t)n;
    DevBuf dx, dy, dl;
    HIP_TRY(c, hipMalloc(&dx.p, np * sizeof(double)));
    HIP_TRY(c, hipMalloc(&dy.p, np * sizeof(double)));
    HIP_TRY(c, hipMalloc(&dl.p, np * sizeof(int)));
    HIP_TRY(c, hipMemcpy(dx.p, x, np * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(dy.p, y, np * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemsetAsync(dl.p, 0, np * sizeof(int), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    tracers_free(c);
    c->tr_x = (double*)dx.p;
    c->tr_y = (double*)dy.p;
    c->tr_laps = (int*)dl.p;
    dx.p = dy.p = dl.p = nullptr;
    c->tr_n = n;
    c->tr_ev.stride = stride;
    c->tr_ev.arm(c->t);
    return IBLB_OK;
}

int iblb_get_tracers(iblb_ctx* c, double* x, double* y, int* laps) {
    if (!c) return IBLB_ERR_ARG;
    if (c->tr_n == 0) return IBLB_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t np = (size_t)c->tr_n;
    return read_back(c, {{x, c->tr_x, np * sizeof(double)},
                         {y, c->tr_y, np * sizeof(double)},
                         {laps, c->tr_laps, np * sizeof(int)}});
}

int iblb_tracer_count(iblb_ctx* c, long long* n, int* stride, long long* updates) {
    if (!c) return IBLB_ERR_ARG;
    if (n) *n = c->tr_n;
    if (stride) *stride = c->tr_ev.stride;
    if (updates) *updates = c->tr_ev.count;
    return IBLB_OK;
}

// ---- the tracers' motion model ----------------------------------------------------------------------
int iblb_set_tracer_model(iblb_ctx* c, const iblb_tracer_model* m, const int* status0, const long long* iteration0) {
    if (!c) return IBLB_ERR_ARG;
    if (m) {
        if (!(std::isfinite(m->diffusivity) && m->diffusivity >= 0.0))
            return fail(c, IBLB_ERR_ARG, "iblb_set_tracer_model: diffusivity must be finite and >= 0");
        if (!(std::isfinite(m->drift[0]) && std::isfinite(m->drift[1])))
            return fail(c, IBLB_ERR_ARG, "iblb_set_tracer_model: drift must be finite");
        for (int w : {m->wall[0], m->wall[1]})
            if (w != IBLB_TRACER_WALL_CLAMP && w != IBLB_TRACER_WALL_REFLECT && w != IBLB_TRACER_WALL_ABSORB)
                return fail(c, IBLB_ERR_ARG, "iblb_set_tracer_model: wall: an unknown IBLB_TRACER_WALL_* kind");
        if ((status0 == nullptr) != (iteration0 == nullptr))
            return fail(c, IBLB_ERR_ARG, "iblb_set_tracer_model: status0 and iteration0 go together: both or neither");
    }
    if (c->tr_n == 0) return fail(c, IBLB_ERR_STATE, "iblb_set_tracer_model: no tracers are set (iblb_set_tracers)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!m) {
        tracer_model_free(c);
        return IBLB_OK;
    }
    const size_t np = (size_t)c->tr_n;
    std::vector<int> st(np, IBLB_TRACER_ALIVE);
    std::vector<long long> hit(np, -1);
    if (status0) {
        std::vector<double> y(np);
        HIP_TRY(c, hipMemcpy(y.data(), c->tr_y, np * sizeof(double), hipMemcpyDeviceToHost));
        const double ytop = (double)(c->ny - 1);
        for (size_t p = 0; p < np; ++p) {
            const int s = status0[p];
            if (s != IBLB_TRACER_ALIVE && s != IBLB_TRACER_AT_BOTTOM && s != IBLB_TRACER_AT_TOP)
                return fail(c, IBLB_ERR_ARG, "iblb_set_tracer_model: status0[" + std::to_string(p) + "] is not an IBLB_TRACER_* status");
            if (s != IBLB_TRACER_ALIVE && y[p] != (s == IBLB_TRACER_AT_BOTTOM ? 0.0 : ytop))
                return fail(c, IBLB_ERR_ARG, "iblb_set_tracer_model: status0[" + std::to_string(p) + "] is deposited, but the tracer is not on that wall's row");
            st[p] = s;
            if (s != IBLB_TRACER_ALIVE) hit[p] = iteration0[p];
        }
    }
    // the new arrays first: a failed allocation leaves the previous model and fates as they were
    DevBuf ds, dh, dd;
    HIP_TRY(c, hipMalloc(&ds.p, np * sizeof(int)));
    HIP_TRY(c, hipMalloc(&dh.p, np * sizeof(long long)));
    HIP_TRY(c, hipMalloc(&dd.p, 2 * (size_t)c->ncol * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemcpy(ds.p, st.data(), np * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(dh.p, hit.data(), np * sizeof(long long), hipMemcpyHostToDevice));
    tracer_model_free(c);
    c->tr_status = (int*)ds.p;
    c->tr_hit = (long long*)dh.p;
    c->tr_dep = (unsigned long long*)dd.p;
    ds.p = dh.p = dd.p = nullptr;
    c->tr_model = *m;
    c->tr_amp = std::sqrt(6.0 * m->diffusivity * (double)c->tr_ev.stride);
    return IBLB_OK;
}

// the per-column deposit counts of both walls, counted on the device: host [2 ncol], bottom then top
static int tracer_deposit_counts(iblb_ctx* c, std::vector<unsigned long long>* host) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_particle_deposit((long)c->tr_n, c->ncol, c->tr_x, c->tr_status, c->tr_dep, c->stream));
    host->resize(2 * (size_t)c->ncol);
    return read_back(c, host->data(), c->tr_dep, host->size() * sizeof(unsigned long long));
}

int iblb_tracer_model_info(iblb_ctx* c, iblb_tracer_model* m, int* present, long long counts[3]) {
    if (!c) return IBLB_ERR_ARG;
    long long k[3] = {0, 0, 0};
    if (counts && c->tr_status) {
        std::vector<unsigned long long> dep;
        int rc = tracer_deposit_counts(c, &dep);
        if (rc) return rc;
        for (int i = 0; i < c->ncol; ++i) {
            k[1] += (long long)dep[i];
            k[2] += (long long)dep[(size_t)c->ncol + i];
        }
        k[0] = c->tr_n - k[1] - k[2];
    }
    if (m) *m = c->tr_model;
    if (present) *present = c->tr_status ? 1 : 0;
    if (counts) std::copy(k, k + 3, counts);
    return IBLB_OK;
}

int iblb_get_tracer_fates(iblb_ctx* c, int* status, long long* iteration) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->tr_status) return fail(c, IBLB_ERR_STATE, "iblb_get_tracer_fates: no model is set (iblb_set_tracer_model)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t np = (size_t)c->tr_n;
    return read_back(c, {{status, c->tr_status, np * sizeof(int)}, {iteration, c->tr_hit, np * sizeof(long long)}});
}

int iblb_get_tracer_deposits(iblb_ctx* c, long long* bottom, long long* top) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->tr_status) return fail(c, IBLB_ERR_STATE, "iblb_get_tracer_deposits: no model is set (iblb_set_tracer_model)");
    std::vector<unsigned long long> dep;
    int rc = tracer_deposit_counts(c, &dep);
    if (rc) return rc;
    for (int i = 0; i < c->ncol; ++i) {
        if (bottom) bottom[i] = (long long)dep[i];
        if (top) top[i] = (long long)dep[(size_t)c->ncol + i];
    }
    return IBLB_OK;
}

// ---- time- and phase-averaged fields ----------------------------------------------------------------
int iblb_set_average(iblb_ctx* c, const iblb_window* w, unsigned fields, int stride, int nbins, unsigned flags) {
    if (!c) return IBLB_ERR_ARG;
    const bool remove = fields == 0 && !w;
    int rc;
    if (!remove) {
        if ((rc = check_fields(c, fields))) return rc;
        if (flags & ~(unsigned)(IBLB_AVG_SQ | IBLB_AVG_UXUY)) return fail(c, IBLB_ERR_ARG, "flags: an unknown IBLB_AVG_* bit");
        if ((flags & IBLB_AVG_UXUY) && (fields & (IBLB_FIELD_UX | IBLB_FIELD_UY)) != (IBLB_FIELD_UX | IBLB_FIELD_UY))
            return fail(c, IBLB_ERR_ARG, "IBLB_AVG_UXUY needs both IBLB_FIELD_UX and IBLB_FIELD_UY");
        if (stride < 1) return fail(c, IBLB_ERR_ARG, "stride must be >= 1");
        if (nbins < 1) return fail(c, IBLB_ERR_ARG, "nbins must be >= 1");
    }
    iblb_window win;
    int lo = 0, nxl = 0;
    if ((rc = window_part(c, w, &win, &lo, &nxl))) return rc;
    if (!single_slab(c))
        return fail(c, IBLB_ERR_UNSUPPORTED,
                    "iblb_set_average: a lone slab only (averaging on the slabs of a group is not built)");
    if (!remove && (rc = check_scalar_fields(c, fields))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (remove) {
        average_free(c);
        return IBLB_OK;
    }
    // the new accumulators first: a failed allocation leaves the previous set as it was
    const int nf = __builtin_popcount(fields);
    const int planes = nf * ((flags & IBLB_AVG_SQ) ? 2 : 1) + ((flags & IBLB_AVG_UXUY) ? 1 : 0);
    const long long cells = (long long)win.nx * win.ny;  // at most the lattice's
    if (cells > LLONG_MAX / (long long)sizeof(double) / planes / nbins)
        return fail(c, IBLB_ERR_NOMEM, "iblb_set_average: the accumulators exceed the address space");
    const size_t bytes = (size_t)cells * planes * nbins * sizeof(double);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, bytes));
    HIP_TRY(c, hipMemsetAsync(d.p, 0, bytes, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    average_free(c);
    c->av_buf = (double*)d.p;
    d.p = nullptr;
    c->av_win = win;
    c->av_fields = fields;
    c->av_flags = flags;
    c->av_nbins = nbins;
    c->av_planes = planes;
    c->av_ev.stride = stride;
    c->av_ev.arm(c->t);
    c->av_count.assign((size_t)nbins, 0);
    return IBLB_OK;
}

int iblb_reset_average(iblb_ctx* c) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->av_fields) return fail(c, IBLB_ERR_STATE, "iblb_reset_average: no averaging is set");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemsetAsync(c->av_buf, 0, (size_t)c->av_nbins * average_bin_elems(c) * sizeof(double), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->av_ev.count = 0;
    c->av_ev.arm(c->t);
    c->av_count.assign((size_t)c->av_nbins, 0);
    return IBLB_OK;
}

int iblb_get_average(iblb_ctx* c, int bin, double* sum, double* sum_sq, double* sum_uxuy, long long* samples) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->av_fields) return fail(c, IBLB_ERR_STATE, "iblb_get_average: no averaging is set");
    if (bin < 0 || bin >= c->av_nbins) return fail(c, IBLB_ERR_ARG, "bin is outside [0, nbins)");
    if (sum_sq && !(c->av_flags & IBLB_AVG_SQ)) return fail(c, IBLB_ERR_ARG, "sum_sq was not requested (IBLB_AVG_SQ)");
    if (sum_uxuy && !(c->av_flags & IBLB_AVG_UXUY))
        return fail(c, IBLB_ERR_ARG, "sum_uxuy was not requested (IBLB_AVG_UXUY)");
    if (sum || sum_sq || sum_uxuy) {
        HIP_TRY(c, hipSetDevice(c->device));
        // the whole bin transposed into the ABI's layout on the device, then whole planes copied
        const size_t plane = (size_t)c->av_win.nx * c->av_win.ny, n = average_bin_elems(c);
        const size_t nf = (size_t)__builtin_popcount(c->av_fields);
        DevBuf d;
        HIP_TRY(c, hipMalloc(&d.p, n * sizeof(double)));
        HIP_TRY(c, launch_average_readout(c->av_buf + (size_t)bin * n, c->av_win.nx, c->av_win.ny, c->av_planes,
                                          (double*)d.p, c->stream));
        const double* t = (const double*)d.p;
        int rc = read_back(c, {{sum, t, nf * plane * sizeof(double)},
                               {sum_sq, t + nf * plane, nf * plane * sizeof(double)},
                               {sum_uxuy, t + (size_t)(c->av_planes - 1) * plane, plane * sizeof(double)}});
        if (rc) return rc;
    }
    if (samples) *samples = c->av_count[(size_t)bin];
    return IBLB_OK;
}

int iblb_average_info(iblb_ctx* c, iblb_window* w, unsigned* fields, int* stride, int* nbins, unsigned* flags,
                      long long* samples_total) {
    if (!c) return IBLB_ERR_ARG;
    if (w) *w = c->av_win;
    if (fields) *fields = c->av_fields;
    if (stride) *stride = c->av_ev.stride;
    if (nbins) *nbins = c->av_nbins;
    if (flags) *flags = c->av_flags;
    if (samples_total) *samples_total = c->av_ev.count;
    return IBLB_OK;
}

// ---- history recorder -----------------------------------------------------------------------------------
int iblb_set_history(iblb_ctx* c, long long n, const double* x, const double* y, unsigned fields, int stride,
                     long long capacity, unsigned flags) {
    if (!c) return IBLB_ERR_ARG;
    if (flags & ~(unsigned)IBLB_HIST_TRACERS) return fail(c, IBLB_ERR_ARG, "flags: an unknown IBLB_HIST_* bit");
    const bool follow = (flags & IBLB_HIST_TRACERS) != 0;
    if (!follow && n < 0) return fail(c, IBLB_ERR_ARG, "n is negative");
    const bool remove = !follow && n == 0;
    int rc;
    if (!remove) {
        if (stride < 1) return fail(c, IBLB_ERR_ARG, "stride must be >= 1");
        if (capacity < 1) return fail(c, IBLB_ERR_ARG, "capacity must be >= 1");
        if (!follow && (!x || !y)) return fail(c, IBLB_ERR_ARG, "x or y is NULL");
        if (fields & ~(IBLB_FIELD_ALL | IBLB_FIELD_SCALAR)) return fail(c, IBLB_ERR_ARG, "fields: an unknown IBLB_FIELD_* bit");
        if (!follow && (rc = check_fields(c, fields))) return rc;
        if (!single_slab(c)) return group_refused(c, "iblb_set_history");
        if (!follow && (rc = check_positions(c, n, x, y))) return rc;
        if ((rc = check_scalar_fields(c, fields))) return rc;
        if (follow && c->tr_n == 0)
            return fail(c, IBLB_ERR_STATE, "iblb_set_history: IBLB_HIST_TRACERS without tracers (iblb_set_tracers)");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (remove) {
        history_free(c);
        return IBLB_OK;
    }
    // the new buffers first: a failed allocation leaves the previous history as it was
    const long long np = follow ? c->tr_n : n;
    const int planes = __builtin_popcount(fields) + (follow ? 3 : 0);
    const long long limit = LLONG_MAX / (long long)sizeof(double);
    if (np > limit / planes / 16 || capacity > (limit - (8LL * planes + 2) * np) / (planes * np))
        return fail(c, IBLB_ERR_NOMEM, "iblb_set_history: the ring exceeds the address space");
    const size_t e = (size_t)planes * (size_t)np;
    const size_t ring = (size_t)capacity * e, total = ring + 8 * e + (follow ? 0 : 2 * (size_t)np);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, total * sizeof(double)));
    double* buf = (double*)d.p;
    std::vector<long long> iter;
    try {
        iter.assign((size_t)capacity, 0);
    } catch (const std::bad_alloc&) {
        return fail(c, IBLB_ERR_NOMEM, "iblb_set_history: no host memory for the slots' iterations");
    }
    const std::vector<double> blank = history_stats_blank(e);
    HIP_TRY(c, hipMemsetAsync(buf, 0, ring * sizeof(double), c->stream));
    HIP_TRY(c, hipMemcpyAsync(buf + ring, blank.data(), 8 * e * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (!follow) {
        HIP_TRY(c, hipMemcpyAsync(buf + ring + 8 * e, x, (size_t)np * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(buf + ring + 8 * e + np, y, (size_t)np * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    history_free(c);
    c->hi_buf = buf;
    d.p = nullptr;
    c->hi_n = np;
    c->hi_cap = capacity;
    c->hi_fields = fields;
    c->hi_flags = flags;
    c->hi_planes = planes;
    c->hi_iter.swap(iter);
    c->hi_ev.stride = stride;
    c->hi_ev.arm(c->t);
    return IBLB_OK;
}

int iblb_reset_history(iblb_ctx* c) {
    if (!c) return IBLB_ERR_ARG;
    if (c->hi_n == 0) return fail(c, IBLB_ERR_STATE, "iblb_reset_history: no history is set");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t e = history_entries(c);
    const std::vector<double> blank = history_stats_blank(e);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(history_stats_base(c), blank.data(), 8 * e * sizeof(double), hipMemcpyHostToDevice));
    c->hi_ev.count = 0;
    c->hi_ev.arm(c->t);
    return IBLB_OK;
}

int iblb_get_history(iblb_ctx* c, long long first, long long count, double* out, long long* iterations) {
    if (!c) return IBLB_ERR_ARG;
    if (c->hi_n == 0) return fail(c, IBLB_ERR_STATE, "iblb_get_history: no history is set");
    if (!out && !iterations) return fail(c, IBLB_ERR_ARG, "out and iterations are both NULL");
    const long long recorded = c->hi_ev.count, oldest = std::max(0LL, recorded - c->hi_cap);
    if (count < 0 || first < oldest || first > recorded || count > recorded - first)
        return fail(c, IBLB_ERR_ARG, "records [first, first + count) are not all in the ring: need first >= max(0, recorded - "
                                     "capacity), count >= 0, first + count <= recorded");
    if (count == 0) return IBLB_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // at most two contiguous runs of the ring: slots [s0, s0 + n1), then [0, count - n1)
    const size_t e = history_entries(c);
    const long long s0 = first % c->hi_cap, n1 = std::min(count, c->hi_cap - s0);
    if (out) {
        int rc = read_back(c, {{out, c->hi_buf + (size_t)s0 * e, (size_t)n1 * e * sizeof(double)},
                               {out + (size_t)n1 * e, c->hi_buf, (size_t)(count - n1) * e * sizeof(double)}});
        if (rc) return rc;
    }
    if (iterations)
        for (long long r = 0; r < count; ++r) iterations[r] = c->hi_iter[(size_t)((first + r) % c->hi_cap)];
    return IBLB_OK;
}

int iblb_get_history_stats(iblb_ctx* c, long long* count, long long* nonfinite, double* sum, double* sum_sq, double* min,
                           double* max, long long* min_rec, long long* max_rec) {
    if (!c) return IBLB_ERR_ARG;
    if (c->hi_n == 0) return fail(c, IBLB_ERR_STATE, "iblb_get_history_stats: no history is set");
    if (!count && !nonfinite && !sum && !sum_sq && !min && !max && !min_rec && !max_rec)
        return fail(c, IBLB_ERR_ARG, "every output is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const HistoryStats s = history_stats(c);
    const size_t nb = history_entries(c) * sizeof(double);
    return read_back(c, {{count, s.count, nb}, {nonfinite, s.nonfinite, nb}, {sum, s.sum, nb}, {sum_sq, s.sum_sq, nb},
                         {min, s.min, nb}, {max, s.max, nb}, {min_rec, s.min_rec, nb}, {max_rec, s.max_rec, nb}});
}

int iblb_get_history_points(iblb_ctx* c, double* x, double* y) {
    if (!c) return IBLB_ERR_ARG;
    if (c->hi_n == 0) return fail(c, IBLB_ERR_STATE, "iblb_get_history_points: no history is set");
    if (c->hi_flags & IBLB_HIST_TRACERS)
        return fail(c, IBLB_ERR_STATE, "iblb_get_history_points: the history follows the tracers (iblb_get_tracers)");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nb = (size_t)c->hi_n * sizeof(double);
    return read_back(c, {{x, history_xy(c), nb}, {y, history_xy(c) + c->hi_n, nb}});
}

int iblb_history_info(iblb_ctx* c, long long* n, unsigned* fields, int* stride, long long* capacity, unsigned* flags,
                      long long* recorded) {
    if (!c) return IBLB_ERR_ARG;
    const bool set = c->hi_n > 0;
    if (n) *n = c->hi_n;
    if (fields) *fields = c->hi_fields;
    if (stride) *stride = set ? c->hi_ev.stride : 0;
    if (capacity) *capacity = c->hi_cap;
    if (flags) *flags = c->hi_flags;
    if (recorded) *recorded = set ? c->hi_ev.count : 0;
    return IBLB_OK;
}

// ---- passive scalar -----------------------------------------------------------------------------------
int iblb_set_scalar(iblb_ctx* c, const iblb_scalar* cfg, const double* c0, const double* g0) {
    if (!c) return IBLB_ERR_ARG;
    if (cfg) {
        if (!std::isfinite(cfg->tau) || !(cfg->tau > 0.5)) return fail(c, IBLB_ERR_ARG, "tau must be finite and > 0.5");
        if (cfg->stride < 1) return fail(c, IBLB_ERR_ARG, "stride must be >= 1");
        for (int k = 0; k < 2; ++k) {
            if (cfg->wall_kind[k] != IBLB_SCALAR_WALL_NOFLUX && cfg->wall_kind[k] != IBLB_SCALAR_WALL_VALUE)
                return fail(c, IBLB_ERR_ARG, "wall_kind: an unknown IBLB_SCALAR_WALL_* value");
            if (cfg->wall_kind[k] == IBLB_SCALAR_WALL_VALUE && !std::isfinite(cfg->wall_value[k]))
                return fail(c, IBLB_ERR_ARG, "wall_value must be finite where the wall kind is IBLB_SCALAR_WALL_VALUE");
        }
        if ((c0 != nullptr) == (g0 != nullptr)) return fail(c, IBLB_ERR_ARG, "exactly one of c0 and g0 must be given");
        if (!single_slab(c))
            return fail(c, IBLB_ERR_UNSUPPORTED,
                        "iblb_set_scalar: a lone slab only (the scalar on the slabs of a group is not built)");
    }
    if (!cfg && (c->av_fields & IBLB_FIELD_SCALAR))
        return fail(c, IBLB_ERR_STATE,
                    "iblb_set_scalar: the current average samples the scalar; remove or replace the average first");
    if (!cfg && (c->hi_fields & IBLB_FIELD_SCALAR))
        return fail(c, IBLB_ERR_STATE,
                    "iblb_set_scalar: the current history records the scalar; remove or replace the history first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!cfg) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        scalar_free(c);
        return IBLB_OK;
    }
    // the state the equilibrium is taken at (c0), as a reader sees it
    int rc = band_join(c);
    if (rc || (rc = prepare_read(c))) return rc;
    // the new buffers first: a failed allocation leaves the previous scalar as it was
    const ScalarGeom S = scalar_geom(c);
    const size_t N = (size_t)c->ncol * c->ny, planes_in = c0 ? 1 : 5;
    if ((size_t)S.plane > SIZE_MAX / sizeof(double) / 12)
        return fail(c, IBLB_ERR_NOMEM, "iblb_set_scalar: the populations exceed the address space");
    DevBuf d, in;
    HIP_TRY(c, hipMalloc(&d.p, 12 * (size_t)S.plane * sizeof(double)));
    HIP_TRY(c, hipMalloc(&in.p, planes_in * N * sizeof(double)));
    double* buf = (double*)d.p;
    HIP_TRY(c, hipMemsetAsync(buf, 0, 12 * (size_t)S.plane * sizeof(double), c->stream));
    HIP_TRY(c, hipMemcpyAsync(in.p, c0 ? c0 : g0, planes_in * N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_scalar_in((const double*)in.p, S, (int)planes_in, buf, c->stream));
    if (c0) {
        const FieldsArgs a = point_args(c, IBLB_FIELD_UX | IBLB_FIELD_UY);
        HIP_TRY(c, with_state(c, [&](auto* g, auto H) { return launch_scalar_init(g, c->L, H, a, S, buf, buf, c->stream); }));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scalar_free(c);
    c->sc_alloc = buf;
    d.p = nullptr;
    c->sc_g[0] = buf;
    c->sc_g[1] = buf + 5 * S.plane;
    c->sc_uv = buf + 10 * S.plane;
    c->sc_cur = 0;
    c->sc_cfg = *cfg;
    c->sc_ev.stride = cfg->stride;
    c->sc_ev.arm(c->t);
    return IBLB_OK;
}

int iblb_get_scalar(iblb_ctx* c, const iblb_window* w, double* out) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_alloc) return fail(c, IBLB_ERR_STATE, "iblb_get_scalar: no scalar is set");
    iblb_window win;
    int lo = 0, nxl = 0, rc;
    if ((rc = window_part(c, w, &win, &lo, &nxl))) return rc;
    if (!out) return fail(c, IBLB_ERR_ARG, "c is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nb = (size_t)win.nx * win.ny * sizeof(double);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, nb));
    HIP_TRY(c, launch_scalar_out(c->sc_g[c->sc_cur], scalar_geom(c), win.x0, win.y0, win.nx, win.ny, win.sx, win.sy,
                                 (double*)d.p, c->stream));
    return read_back(c, out, d.p, nb);
}

int iblb_get_scalar_populations(iblb_ctx* c, double* g) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_alloc) return fail(c, IBLB_ERR_STATE, "iblb_get_scalar_populations: no scalar is set");
    if (!g) return fail(c, IBLB_ERR_ARG, "g is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nb = 5 * (size_t)c->ncol * c->ny * sizeof(double);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, nb));
    HIP_TRY(c, launch_scalar_populations_out(c->sc_g[c->sc_cur], scalar_geom(c), (double*)d.p, c->stream));
    return read_back(c, g, d.p, nb);
}

int iblb_get_scalar_wall_flux(iblb_ctx* c, double* bottom, double* top) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_alloc) return fail(c, IBLB_ERR_STATE, "iblb_get_scalar_wall_flux: no scalar is set");
    if (!bottom && !top) return fail(c, IBLB_ERR_ARG, "bottom and top are both NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nb = (size_t)c->ncol * sizeof(double);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, 2 * nb));
    HIP_TRY(c, launch_scalar_wall_flux(c->sc_g[c->sc_cur], scalar_geom(c), scalar_rule(c->sc_cfg), scalar_source(c),
                                       (double*)d.p, c->stream));
    return read_back(c, {{bottom, d.p, nb}, {top, (double*)d.p + c->ncol, nb}});
}

int iblb_scalar_info(iblb_ctx* c, iblb_scalar* cfg, long long* updates) {
    if (!c) return IBLB_ERR_ARG;
    if (cfg) *cfg = c->sc_cfg;
    if (updates) *updates = c->sc_ev.count;
    return IBLB_OK;
}

// a_k[x] of iblb_set_scalar_uptake from the rate k: 2.0 - 2.0/(1.0 + 3.0*k), every operation in double and rounded
// once.  The volatiles keep the host compiler from contracting 1.0 + 3.0*k into one fused operation.
static double uptake_coefficient(double k) {
    volatile double t = 3.0 * k;
    volatile double d = 1.0 + t;
    volatile double q = 2.0 / d;
    return 2.0 - q;
}

// ---- the scalar's source ------------------------------------------------------------------------------
static bool all_finite(const double* a, size_t n) {
    for (size_t j = 0; j < n; ++j)
        if (!std::isfinite(a[j])) return false;
    return true;
}

int iblb_set_scalar_source(iblb_ctx* c, const iblb_scalar_source* src) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_alloc)
        return fail(c, IBLB_ERR_STATE, single_slab(c) ? "iblb_set_scalar_source: no scalar is set (iblb_set_scalar)"
                                                      : "iblb_set_scalar_source: a slab of a group holds no scalar");
    const size_t N = (size_t)c->ncol * c->ny, ncol = (size_t)c->ncol;
    if (src) {
        if (!std::isfinite(src->decay) || src->decay < 0.0) return fail(c, IBLB_ERR_ARG, "decay must be finite and >= 0");
        if (src->source && !all_finite(src->source, N)) return fail(c, IBLB_ERR_ARG, "source holds a non-finite entry");
        for (int k = 0; k < 2; ++k) {
            const bool value = c->sc_cfg.wall_kind[k] == IBLB_SCALAR_WALL_VALUE;
            if (src->wall_flux[k] && value)
                return fail(c, IBLB_ERR_ARG, "wall_flux is given for a wall of kind IBLB_SCALAR_WALL_VALUE");
            if (src->wall_value[k] && !value)
                return fail(c, IBLB_ERR_ARG, "wall_value is given for a wall of kind IBLB_SCALAR_WALL_NOFLUX");
            if (src->wall_flux[k] && !all_finite(src->wall_flux[k], ncol))
                return fail(c, IBLB_ERR_ARG, "wall_flux holds a non-finite entry");
            if (src->wall_value[k] && !all_finite(src->wall_value[k], ncol))
                return fail(c, IBLB_ERR_ARG, "wall_value holds a non-finite entry");
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!src) {
        scalar_source_free(c);
        return IBLB_OK;
    }
    // the four wall arrays side by side; what the call leaves NULL is held as the value the rule then uses
    std::vector<double> walls(4 * ncol, 0.0);
    unsigned present = 1u | (src->source ? 2u : 0u);
    for (int k = 0; k < 2; ++k) {
        if (src->wall_flux[k]) {
            std::copy(src->wall_flux[k], src->wall_flux[k] + ncol, walls.begin() + (size_t)k * ncol);
            present |= 4u << k;
        }
        if (src->wall_value[k]) {
            std::copy(src->wall_value[k], src->wall_value[k] + ncol, walls.begin() + (size_t)(2 + k) * ncol);
            present |= 16u << k;
        } else if (c->sc_cfg.wall_kind[k] == IBLB_SCALAR_WALL_VALUE) {
            std::fill_n(walls.begin() + (size_t)(2 + k) * ncol, ncol, c->sc_cfg.wall_value[k]);
        }
    }
    // the new buffers first: a failed allocation leaves the previous source as it was
    const ScalarGeom S = scalar_geom(c);
    DevBuf df, dw, in;
    HIP_TRY(c, hipMalloc(&df.p, (size_t)S.plane * sizeof(double)));
    HIP_TRY(c, hipMalloc(&dw.p, 4 * ncol * sizeof(double)));
    HIP_TRY(c, hipMemsetAsync(df.p, 0, (size_t)S.plane * sizeof(double), c->stream));
    if (src->source) {
        HIP_TRY(c, hipMalloc(&in.p, N * sizeof(double)));
        HIP_TRY(c, hipMemcpyAsync(in.p, src->source, N * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, launch_scalar_in((const double*)in.p, S, 1, (double*)df.p, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(dw.p, walls.data(), 4 * ncol * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scalar_source_free(c);
    c->sc_src_field = (double*)df.p;
    c->sc_src_walls = (double*)dw.p;
    df.p = dw.p = nullptr;
    c->sc_src_decay = src->decay;
    c->sc_src_present = present;
    return IBLB_OK;
}

int iblb_scalar_source_info(iblb_ctx* c, double* decay, unsigned* present) {
    if (!c) return IBLB_ERR_ARG;
    if (decay) *decay = c->sc_src_decay;
    if (present) *present = c->sc_src_present;
    return IBLB_OK;
}

int iblb_get_scalar_source(iblb_ctx* c, double* source) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_src_present) return fail(c, IBLB_ERR_STATE, "iblb_get_scalar_source: no source is set");
    if (!source) return fail(c, IBLB_ERR_ARG, "source is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nb = (size_t)c->ncol * c->ny * sizeof(double);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, nb));
    HIP_TRY(c, launch_scalar_plane_out(c->sc_src_field, scalar_geom(c), (double*)d.p, c->stream));
    return read_back(c, source, d.p, nb);
}

// ---- the scalar's uptake ------------------------------------------------------------------------------
int iblb_set_scalar_uptake(iblb_ctx* c, const iblb_scalar_uptake* up) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_alloc)
        return fail(c, IBLB_ERR_STATE, single_slab(c) ? "iblb_set_scalar_uptake: no scalar is set (iblb_set_scalar)"
                                                      : "iblb_set_scalar_uptake: a slab of a group holds no scalar");
    const size_t ncol = (size_t)c->ncol;
    if (up) {
        for (int k = 0; k < 2; ++k) {
            if (!up->rate[k]) continue;
            if (c->sc_cfg.wall_kind[k] == IBLB_SCALAR_WALL_VALUE)
                return fail(c, IBLB_ERR_ARG, "rate is given for a wall of kind IBLB_SCALAR_WALL_VALUE");
            for (size_t x = 0; x < ncol; ++x)
                if (!std::isfinite(up->rate[k][x]) || up->rate[k][x] < 0.0)
                    return fail(c, IBLB_ERR_ARG, "rate holds an entry that is not finite or is negative");
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!up) {
        scalar_uptake_free(c);
        return IBLB_OK;
    }
    // a, total, last side by side; a of a NULL rate array and both accumulators start as zeros
    std::vector<double> host(6 * ncol, 0.0);
    unsigned present = 1u;
    for (int k = 0; k < 2; ++k) {
        if (!up->rate[k]) continue;
        for (size_t x = 0; x < ncol; ++x) host[(size_t)k * ncol + x] = uptake_coefficient(up->rate[k][x]);
        present |= 2u << k;
    }
    // the new buffer first: a failed allocation leaves the previous uptake as it was
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, 6 * ncol * sizeof(double)));
    HIP_TRY(c, hipMemcpyAsync(d.p, host.data(), 6 * ncol * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scalar_uptake_free(c);
    c->sc_up = (double*)d.p;
    d.p = nullptr;
    c->sc_up_present = present;
    return IBLB_OK;
}

int iblb_reset_scalar_uptake(iblb_ctx* c) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_up) return fail(c, IBLB_ERR_STATE, "iblb_reset_scalar_uptake: no uptake is set");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = 2 * (size_t)c->ncol;  // total and last follow a
    HIP_TRY(c, hipMemsetAsync(c->sc_up + n, 0, 2 * n * sizeof(double), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->sc_up_substeps = 0;
    return IBLB_OK;
}

int iblb_get_scalar_uptake(iblb_ctx* c, double* total_bottom, double* total_top, double* last_bottom, double* last_top,
                           long long* substeps) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_up) return fail(c, IBLB_ERR_STATE, "iblb_get_scalar_uptake: no uptake is set");
    if (!total_bottom && !total_top && !last_bottom && !last_top && !substeps)
        return fail(c, IBLB_ERR_ARG, "every output is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const ScalarUptake U = scalar_uptake(c);
    const size_t nb = (size_t)c->ncol * sizeof(double);
    int rc = read_back(c, {{total_bottom, U.total, nb},
                           {total_top, U.total + c->ncol, nb},
                           {last_bottom, U.last, nb},
                           {last_top, U.last + c->ncol, nb}});
    if (rc) return rc;
    if (substeps) *substeps = c->sc_up_substeps;
    return IBLB_OK;
}

int iblb_scalar_uptake_info(iblb_ctx* c, unsigned* present, long long* substeps) {
    if (!c) return IBLB_ERR_ARG;
    if (present) *present = c->sc_up_present;
    if (substeps) *substeps = c->sc_up_substeps;
    return IBLB_OK;
}

// ---- the scalar's open ends in x ----------------------------------------------------------------------
int iblb_set_scalar_ends(iblb_ctx* c, const iblb_scalar_ends* ends) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_alloc)
        return fail(c, IBLB_ERR_STATE, single_slab(c) ? "iblb_set_scalar_ends: no scalar is set (iblb_set_scalar)"
                                                      : "iblb_set_scalar_ends: a slab of a group holds no scalar");
    const size_t ny = (size_t)c->ny;
    if (ends) {
        for (int k = 0; k < 2; ++k) {
            const int kind = ends->kind[k];
            if (kind != IBLB_SCALAR_END_NOFLUX && kind != IBLB_SCALAR_END_VALUE && kind != IBLB_SCALAR_END_OUTFLOW)
                return fail(c, IBLB_ERR_ARG, "kind is none of IBLB_SCALAR_END_NOFLUX, _VALUE, _OUTFLOW");
            if (kind != IBLB_SCALAR_END_VALUE) {
                if (ends->profile[k])
                    return fail(c, IBLB_ERR_ARG, "profile is given for an end that is not of kind IBLB_SCALAR_END_VALUE");
                continue;
            }
            if (!std::isfinite(ends->value[k])) return fail(c, IBLB_ERR_ARG, "value of a _VALUE end is not finite");
            if (ends->profile[k] && !all_finite(ends->profile[k], ny))
                return fail(c, IBLB_ERR_ARG, "profile holds an entry that is not finite");
        }
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!ends) {
        scalar_ends_free(c);
        return IBLB_OK;
    }
    // value, total, last side by side; a NULL profile is the uniform value (0.0 at an end that takes none), and both
    // accumulators start as zeros
    std::vector<double> host(6 * ny, 0.0);
    unsigned present = 1u;
    for (int k = 0; k < 2; ++k) {
        if (ends->kind[k] != IBLB_SCALAR_END_VALUE) continue;
        for (size_t y = 0; y < ny; ++y) host[(size_t)k * ny + y] = ends->profile[k] ? ends->profile[k][y] : ends->value[k];
        if (ends->profile[k]) present |= 2u << k;
    }
    // the new buffer first: a failed allocation leaves the previous ends as they were
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, 6 * ny * sizeof(double)));
    HIP_TRY(c, hipMemcpyAsync(d.p, host.data(), 6 * ny * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    scalar_ends_free(c);
    c->sc_end = (double*)d.p;
    d.p = nullptr;
    for (int k = 0; k < 2; ++k) {
        c->sc_end_kind[k] = ends->kind[k];
        c->sc_end_value[k] = ends->value[k];
    }
    c->sc_end_present = present;
    return IBLB_OK;
}

int iblb_reset_scalar_ends(iblb_ctx* c) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_end) return fail(c, IBLB_ERR_STATE, "iblb_reset_scalar_ends: no ends are set");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = 2 * (size_t)c->ny;  // total and last follow value
    HIP_TRY(c, hipMemsetAsync(c->sc_end + n, 0, 2 * n * sizeof(double), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->sc_end_substeps = 0;
    return IBLB_OK;
}

int iblb_get_scalar_ends(iblb_ctx* c, double* total_left, double* total_right, double* last_left, double* last_right,
                         long long* substeps) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_end) return fail(c, IBLB_ERR_STATE, "iblb_get_scalar_ends: no ends are set");
    if (!total_left && !total_right && !last_left && !last_right && !substeps)
        return fail(c, IBLB_ERR_ARG, "every output is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const ScalarEnds E = scalar_ends(c);
    const size_t nb = (size_t)c->ny * sizeof(double);
    int rc = read_back(c, {{total_left, E.total, nb},
                           {total_right, E.total + c->ny, nb},
                           {last_left, E.last, nb},
                           {last_right, E.last + c->ny, nb}});
    if (rc) return rc;
    if (substeps) *substeps = c->sc_end_substeps;
    return IBLB_OK;
}

int iblb_scalar_ends_info(iblb_ctx* c, int kind[2], double value[2], unsigned* present, long long* substeps) {
    if (!c) return IBLB_ERR_ARG;
    if (c->sc_end_present) {
        for (int k = 0; k < 2; ++k) {
            if (kind) kind[k] = c->sc_end_kind[k];
            if (value) value[k] = c->sc_end_value[k];
        }
    }
    if (present) *present = c->sc_end_present;
    if (substeps) *substeps = c->sc_end_substeps;
    return IBLB_OK;
}

// ---- the scalar's transport gauges --------------------------------------------------------------------
// n entries strictly ascending within 0 .. hi
static bool gauge_list_ok(int n, const int* v, int hi) {
    for (int k = 0; k < n; ++k)
        if (v[k] < 0 || v[k] > hi || (k > 0 && v[k] <= v[k - 1])) return false;
    return true;
}

// sc_gau for the checked lists station and level, in *d: the four totals (zeros, or `totals` from the host) and the
// index arrays of ScalarGauges.  Synchronises the context's stream.
static int gauges_buffer(iblb_ctx* c, int n_stations, const int* station, int n_levels, const int* level,
                         const double* totals, DevBuf* d) {
    const int ncol = c->ncol, ny = c->ny;
    // the index arrays of ScalarGauges: {own, the left neighbour's} per column, {own, the row below's} per row
    std::vector<int> col(2 * (size_t)ncol, -1), row(2 * (size_t)ny, -1);
    for (int k = 0; k < n_stations; ++k) {
        const int x = station[k];
        col[2 * (size_t)x] = k;
        col[2 * (size_t)(x + 1 < ncol ? x + 1 : 0) + 1] = k;
    }
    for (int k = 0; k < n_levels; ++k) {
        const int y = level[k];
        row[2 * (size_t)y] = k;
        row[2 * (size_t)(y + 1) + 1] = k;
    }
    const size_t nt = 2 * ((size_t)n_stations * ny + (size_t)n_levels * ncol);
    const size_t nb = nt * sizeof(double) + 2 * ((size_t)ncol + ny) * sizeof(int);
    HIP_TRY(c, hipMalloc(&d->p, nb));
    int* idx = (int*)((double*)d->p + nt);
    if (totals) HIP_TRY(c, hipMemcpyAsync(d->p, totals, nt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    else HIP_TRY(c, hipMemsetAsync(d->p, 0, nt * sizeof(double), c->stream));
    HIP_TRY(c, hipMemcpyAsync(idx, col.data(), col.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(idx + col.size(), row.data(), row.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return IBLB_OK;
}

int iblb_set_scalar_gauges(iblb_ctx* c, const iblb_scalar_gauges* ga) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_alloc)
        return fail(c, IBLB_ERR_STATE, single_slab(c) ? "iblb_set_scalar_gauges: no scalar is set (iblb_set_scalar)"
                                                      : "iblb_set_scalar_gauges: a slab of a group holds no scalar");
    const int ncol = c->ncol, ny = c->ny;
    if (ga) {
        if (ga->n_stations < 0 || ga->n_stations > ncol) return fail(c, IBLB_ERR_ARG, "n_stations is outside 0 .. XDIM");
        if (ga->n_levels < 0 || ga->n_levels > ny - 1) return fail(c, IBLB_ERR_ARG, "n_levels is outside 0 .. YDIM-1");
        if (ga->n_stations == 0 && ga->n_levels == 0)
            return fail(c, IBLB_ERR_ARG, "n_stations and n_levels are both 0 (NULL removes the gauges)");
        if (ga->n_stations > 0 && !ga->station) return fail(c, IBLB_ERR_ARG, "station is NULL and n_stations is not 0");
        if (ga->n_levels > 0 && !ga->level) return fail(c, IBLB_ERR_ARG, "level is NULL and n_levels is not 0");
        if (!gauge_list_ok(ga->n_stations, ga->station, ncol - 1))
            return fail(c, IBLB_ERR_ARG, "station must be strictly ascending within 0 .. XDIM-1");
        if (!gauge_list_ok(ga->n_levels, ga->level, ny - 2))
            return fail(c, IBLB_ERR_ARG, "level must be strictly ascending within 0 .. YDIM-2");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!ga) {
        scalar_gauges_free(c);
        return IBLB_OK;
    }
    // the new buffer first: a failed allocation leaves the previous gauges as they were
    DevBuf d;
    int rc = gauges_buffer(c, ga->n_stations, ga->station, ga->n_levels, ga->level, nullptr, &d);
    if (rc) return rc;
    scalar_gauges_free(c);
    c->sc_gau = (double*)d.p;
    d.p = nullptr;
    if (ga->n_stations > 0) c->sc_gau_station.assign(ga->station, ga->station + ga->n_stations);
    if (ga->n_levels > 0) c->sc_gau_level.assign(ga->level, ga->level + ga->n_levels);
    return IBLB_OK;
}

int iblb_reset_scalar_gauges(iblb_ctx* c) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_gau) return fail(c, IBLB_ERR_STATE, "iblb_reset_scalar_gauges: no gauges are set");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemsetAsync(c->sc_gau, 0, scalar_gauges_totals(c) * sizeof(double), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->sc_gau_substeps = 0;
    return IBLB_OK;
}

int iblb_get_scalar_gauges(iblb_ctx* c, double* right, double* left, double* up, double* down, long long* substeps) {
    if (!c) return IBLB_ERR_ARG;
    if (!c->sc_gau) return fail(c, IBLB_ERR_STATE, "iblb_get_scalar_gauges: no gauges are set");
    if (!right && !left && !up && !down && !substeps) return fail(c, IBLB_ERR_ARG, "every output is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const ScalarGauges G = scalar_gauges(c);
    const size_t ns = c->sc_gau_station.size() * (size_t)c->ny * sizeof(double);
    const size_t nl = c->sc_gau_level.size() * (size_t)c->ncol * sizeof(double);
    int rc = read_back(c, {{right, G.right, ns}, {left, G.left, ns}, {up, G.up, nl}, {down, G.down, nl}});
    if (rc) return rc;
    if (substeps) *substeps = c->sc_gau_substeps;
    return IBLB_OK;
}

int iblb_scalar_gauges_info(iblb_ctx* c, int* n_stations, int* station, int* n_levels, int* level,
                            long long* substeps) {
    if (!c) return IBLB_ERR_ARG;
    if (n_stations) *n_stations = (int)c->sc_gau_station.size();
    if (station) std::copy(c->sc_gau_station.begin(), c->sc_gau_station.end(), station);
    if (n_levels) *n_levels = (int)c->sc_gau_level.size();
    if (level) std::copy(c->sc_gau_level.begin(), c->sc_gau_level.end(), level);
    if (substeps) *substeps = c->sc_gau_substeps;
    return IBLB_OK;
}

}  // extern "C"

// ---- observers in checkpoints ---------------------------------------------------------------------------
// The sections' payloads (laid out above the checkpoint code of iblb_ctx.hip) written from and restored into the
// context.  Every lattice-sized array crosses in the layout of its getter, through the getters' own transposes.
namespace iblbh {
namespace {

// a payload under construction: 8-byte integers and doubles, arrays as raw bytes
struct Put {
    std::vector<char>* b;
    void raw(const void* p, size_t n) { b->insert(b->end(), (const char*)p, (const char*)p + n); }
    void i64(long long v) { raw(&v, 8); }
    void f64(double v) { raw(&v, 8); }
    // n bytes from the device (the context's stream synchronised)
    int dev(iblb_ctx* c, const void* d, size_t n) {
        const size_t at = b->size();
        b->resize(at + n);
        if (n) HIP_TRY(c, hipMemcpy(b->data() + at, d, n, hipMemcpyDeviceToHost));
        return IBLB_OK;
    }
};

// a payload being read: every take checks the bytes left; ok stays false after the first short take
struct Get {
    const char* p;
    size_t n, pos = 0;
    bool ok = true;
    bool raw(void* dst, size_t bytes) {
        if (!ok || bytes > n - pos) return ok = false;
        if (bytes) std::memcpy(dst, p + pos, bytes);
        pos += bytes;
        return true;
    }
    long long i64() {
        long long v = 0;
        raw(&v, 8);
        return v;
    }
    double f64() {
        double v = 0.0;
        raw(&v, 8);
        return v;
    }
    // an int64 that must lie in [lo, hi] to be taken as an int
    int i32(long long lo, long long hi) {
        const long long v = i64();
        if (v < lo || v > hi) ok = false;
        return ok ? (int)v : 0;
    }
    template <typename T>
    bool array(std::vector<T>* v, size_t count) {
        if (!ok || count > (n - pos) / sizeof(T)) return ok = false;
        v->resize(count);
        return raw(v->data(), count * sizeof(T));
    }
    bool done() const { return ok && pos == n; }
};

// A schedule in a file: t0, the absolute iteration its runs count from — run number m (from 0) comes after iteration
// t0 + (m + 1) stride — and the runs done.  t0 is the iteration of the set or the reset; iblb_set_state, which keeps
// the count and starts the iterations again, moves it below zero.
long long schedule_t0(const Periodic& ev) { return ev.next - (ev.count + 1) * ev.stride; }

// the schedule (t0, stride, count) of a file saved at iteration t: the next run lies within (t, t + stride]
bool schedule_ok(long long t, long long t0, int stride, long long count, long long* next) {
    long long ahead = 0;
    if (stride < 1 || count < 0 || count == LLONG_MAX) return false;
    if (__builtin_mul_overflow(count + 1, (long long)stride, &ahead) || __builtin_add_overflow(t0, ahead, next)) return false;
    return *next > t && *next - stride <= t;
}

int pack_scalar(iblb_ctx* c, Put w) {
    const size_t ncol = (size_t)c->ncol, ny = (size_t)c->ny, N = ncol * ny;
    const ScalarGeom S = scalar_geom(c);
    const unsigned parts = (c->sc_src_present ? 1u : 0u) | (c->sc_up ? 2u : 0u) | (c->sc_end ? 4u : 0u) | (c->sc_gau ? 8u : 0u);
    for (long long v : {(long long)c->nx, (long long)c->ny, (long long)c->sc_cfg.stride, (long long)c->sc_cfg.wall_kind[0],
                        (long long)c->sc_cfg.wall_kind[1], schedule_t0(c->sc_ev), c->sc_ev.count, (long long)parts})
        w.i64(v);
    for (double v : {c->sc_cfg.tau, c->sc_cfg.wall_value[0], c->sc_cfg.wall_value[1]}) w.f64(v);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, 5 * N * sizeof(double)));
    HIP_TRY(c, launch_scalar_populations_out(c->sc_g[c->sc_cur], S, (double*)d.p, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int rc = w.dev(c, d.p, 5 * N * sizeof(double));
    if (rc) return rc;
    if (parts & 1u) {
        w.i64(c->sc_src_present);
        w.f64(c->sc_src_decay);
        HIP_TRY(c, launch_scalar_plane_out(c->sc_src_field, S, (double*)d.p, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if ((rc = w.dev(c, d.p, N * sizeof(double))) || (rc = w.dev(c, c->sc_src_walls, 4 * ncol * sizeof(double)))) return rc;
    }
    if (parts & 2u) {
        w.i64(c->sc_up_present);
        w.i64(c->sc_up_substeps);
        if ((rc = w.dev(c, c->sc_up, 6 * ncol * sizeof(double)))) return rc;
    }
    if (parts & 4u) {
        for (long long v : {(long long)c->sc_end_kind[0], (long long)c->sc_end_kind[1], (long long)c->sc_end_present,
                            c->sc_end_substeps})
            w.i64(v);
        w.f64(c->sc_end_value[0]);
        w.f64(c->sc_end_value[1]);
        if ((rc = w.dev(c, c->sc_end, 6 * ny * sizeof(double)))) return rc;
    }
    if (parts & 8u) {
        w.i64((long long)c->sc_gau_station.size());
        w.i64((long long)c->sc_gau_level.size());
        w.i64(c->sc_gau_substeps);
        for (int v : c->sc_gau_station) w.i64(v);
        for (int v : c->sc_gau_level) w.i64(v);
        if ((rc = w.dev(c, c->sc_gau, scalar_gauges_totals(c) * sizeof(double)))) return rc;
    }
    return IBLB_OK;
}

int pack_tracers(iblb_ctx* c, Put w) {
    const size_t np = (size_t)c->tr_n;
    for (long long v : {c->tr_n, (long long)c->tr_ev.stride, schedule_t0(c->tr_ev), c->tr_ev.count}) w.i64(v);
    int rc;
    if ((rc = w.dev(c, c->tr_x, np * sizeof(double))) || (rc = w.dev(c, c->tr_y, np * sizeof(double))) ||
        (rc = w.dev(c, c->tr_laps, np * sizeof(int))))
        return rc;
    return IBLB_OK;
}

int pack_average(iblb_ctx* c, Put w) {
    const iblb_window& a = c->av_win;
    for (long long v : {(long long)a.x0, (long long)a.y0, (long long)a.nx, (long long)a.ny, (long long)a.sx, (long long)a.sy,
                        (long long)c->av_fields, (long long)c->av_flags, (long long)c->av_ev.stride, (long long)c->av_nbins,
                        schedule_t0(c->av_ev), c->av_ev.count})
        w.i64(v);
    for (long long v : c->av_count) w.i64(v);
    // every bin transposed into the ABI's layout on the device, as iblb_get_average does
    const size_t n = average_bin_elems(c);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, n * sizeof(double)));
    for (int bin = 0; bin < c->av_nbins; ++bin) {
        HIP_TRY(c, launch_average_readout(c->av_buf + (size_t)bin * n, a.nx, a.ny, c->av_planes, (double*)d.p, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        int rc = w.dev(c, d.p, n * sizeof(double));
        if (rc) return rc;
    }
    return IBLB_OK;
}

int bad(iblb_ctx* c, const char* section, const char* what) {
    return fail(c, IBLB_ERR_ARG, std::string("checkpoint, ") + section + " section: " + what);
}

int parse_scalar(iblb_ctx* c, long long t, Get r, CkScalar* s) {
    const char* const sec = "scalar";
    const size_t nx = (size_t)c->nx, ny = (size_t)c->ny;
    const long long fnx = r.i64(), fny = r.i64();
    if (!r.ok || fnx != c->nx || fny != c->ny) return bad(c, sec, "the lattice differs from the context's");
    s->cfg.stride = r.i32(1, INT_MAX);
    s->cfg.wall_kind[0] = r.i32(IBLB_SCALAR_WALL_NOFLUX, IBLB_SCALAR_WALL_VALUE);
    s->cfg.wall_kind[1] = r.i32(IBLB_SCALAR_WALL_NOFLUX, IBLB_SCALAR_WALL_VALUE);
    if (!r.ok) return bad(c, sec, "stride < 1 or an unknown wall kind");
    s->t0 = r.i64();
    s->events = r.i64();
    s->parts = (unsigned)r.i32(0, 15);
    s->cfg.tau = r.f64();
    s->cfg.wall_value[0] = r.f64();
    s->cfg.wall_value[1] = r.f64();
    long long next = 0;
    if (!r.ok || !schedule_ok(t, s->t0, s->cfg.stride, s->events, &next)) return bad(c, sec, "an inconsistent header or schedule");
    if (!std::isfinite(s->cfg.tau) || !(s->cfg.tau > 0.5)) return bad(c, sec, "tau must be finite and > 0.5");
    for (int k = 0; k < 2; ++k)
        if (s->cfg.wall_kind[k] == IBLB_SCALAR_WALL_VALUE && !std::isfinite(s->cfg.wall_value[k]))
            return bad(c, sec, "the value of a _VALUE wall is not finite");
    if (!r.array(&s->pops, 5 * nx * ny)) return bad(c, sec, "truncated in the populations");
    if (s->parts & 1u) {
        s->src_present = (unsigned)r.i32(1, 63);
        s->src_decay = r.f64();
        if (!r.ok || !(s->src_present & 1u) || !std::isfinite(s->src_decay) || s->src_decay < 0.0)
            return bad(c, sec, "the source's present bits or decay");
        if (!r.array(&s->src_field, nx * ny) || !r.array(&s->src_walls, 4 * nx)) return bad(c, sec, "truncated in the source");
    }
    if (s->parts & 2u) {
        s->up_present = (unsigned)r.i32(1, 7);
        s->up_substeps = r.i64();
        if (!r.ok || !(s->up_present & 1u) || s->up_substeps < 0) return bad(c, sec, "the uptake's present bits or substeps");
        if (!r.array(&s->up, 6 * nx)) return bad(c, sec, "truncated in the uptake");
    }
    if (s->parts & 4u) {
        s->end_kind[0] = r.i32(IBLB_SCALAR_END_NOFLUX, IBLB_SCALAR_END_OUTFLOW);
        s->end_kind[1] = r.i32(IBLB_SCALAR_END_NOFLUX, IBLB_SCALAR_END_OUTFLOW);
        if (!r.ok) return bad(c, sec, "an unknown end kind");
        s->end_present = (unsigned)r.i32(1, 7);
        s->end_substeps = r.i64();
        s->end_value[0] = r.f64();
        s->end_value[1] = r.f64();
        if (!r.ok || !(s->end_present & 1u) || s->end_substeps < 0) return bad(c, sec, "the ends' present bits or substeps");
        for (int k = 0; k < 2; ++k)
            if (s->end_kind[k] == IBLB_SCALAR_END_VALUE && !std::isfinite(s->end_value[k]))
                return bad(c, sec, "the value of a _VALUE end is not finite");
        if (!r.array(&s->end, 6 * ny)) return bad(c, sec, "truncated in the ends");
    }
    if (s->parts & 8u) {
        const int n_st = r.i32(0, c->nx), n_lv = r.i32(0, c->ny - 1);
        s->gau_substeps = r.i64();
        if (!r.ok || (n_st == 0 && n_lv == 0) || s->gau_substeps < 0)
            return bad(c, sec, "the gauges' counts are outside 0 .. XDIM and 0 .. YDIM-1, or both 0");
        for (int k = 0; k < n_st; ++k) s->station.push_back(r.i32(0, c->nx - 1));
        for (int k = 0; k < n_lv; ++k) s->level.push_back(r.i32(0, c->ny - 2));
        if (!r.ok || !gauge_list_ok(n_st, s->station.data(), c->nx - 1) || !gauge_list_ok(n_lv, s->level.data(), c->ny - 2))
            return bad(c, sec, "the gauges' positions must be strictly ascending within the lattice");
        if (!r.array(&s->gau, 2 * ((size_t)n_st * ny + (size_t)n_lv * nx))) return bad(c, sec, "truncated in the gauges");
    }
    if (!r.done()) return bad(c, sec, "its length does not match its header");
    return IBLB_OK;
}

int parse_tracers(iblb_ctx* c, long long t, Get r, CkTracers* s) {
    const char* const sec = "tracer";
    s->n = r.i64();
    s->stride = r.i32(1, INT_MAX);
    s->t0 = r.i64();
    s->updates = r.i64();
    long long next = 0;
    if (!r.ok || s->n < 1 || !schedule_ok(t, s->t0, s->stride, s->updates, &next))
        return bad(c, sec, "n < 1, stride < 1 or an inconsistent schedule");
    if ((unsigned long long)s->n > r.n / 20) return bad(c, sec, "truncated in the positions");
    const size_t np = (size_t)s->n;
    if (!r.array(&s->x, np) || !r.array(&s->y, np) || !r.array(&s->laps, np)) return bad(c, sec, "truncated in the positions");
    if (!r.done()) return bad(c, sec, "its length does not match its header");
    if (check_positions(c, s->n, s->x.data(), s->y.data())) return bad(c, sec, "a position outside the lattice");
    return IBLB_OK;
}

int parse_average(iblb_ctx* c, long long t, Get r, bool scalar, CkAverage* s) {
    const char* const sec = "average";
    int* const w[6] = {&s->win.x0, &s->win.y0, &s->win.nx, &s->win.ny, &s->win.sx, &s->win.sy};
    for (int* p : w) *p = r.i32(0, INT_MAX);
    s->fields = (unsigned)r.i32(1, IBLB_FIELD_ALL | IBLB_FIELD_SCALAR);
    s->flags = (unsigned)r.i32(0, IBLB_AVG_SQ | IBLB_AVG_UXUY);
    s->stride = r.i32(1, INT_MAX);
    s->nbins = r.i32(1, INT_MAX);
    s->t0 = r.i64();
    s->samples = r.i64();
    long long next = 0;
    iblb_window win;
    int lo = 0, nxl = 0;
    if (!r.ok || !schedule_ok(t, s->t0, s->stride, s->samples, &next)) return bad(c, sec, "an inconsistent header or schedule");
    if (window_part(c, &s->win, &win, &lo, &nxl)) return bad(c, sec, "the window leaves the lattice");
    if ((s->fields & ~(IBLB_FIELD_ALL | IBLB_FIELD_SCALAR)) || (s->flags & ~(unsigned)(IBLB_AVG_SQ | IBLB_AVG_UXUY)) ||
        ((s->flags & IBLB_AVG_UXUY) && (s->fields & (IBLB_FIELD_UX | IBLB_FIELD_UY)) != (IBLB_FIELD_UX | IBLB_FIELD_UY)))
        return bad(c, sec, "unknown field or flag bits");
    if ((s->fields & IBLB_FIELD_SCALAR) && !scalar)
        return bad(c, sec, "it samples the scalar and the file holds no scalar section");
    if ((size_t)s->nbins > r.n / 8 || !r.array(&s->count, (size_t)s->nbins)) return bad(c, sec, "truncated in the counts");
    long long total = 0;
    for (long long v : s->count)
        if (v < 0 || __builtin_add_overflow(total, v, &total)) return bad(c, sec, "a negative count");
    if (total != s->samples) return bad(c, sec, "the bins' counts do not add up to the sample count");
    s->planes = __builtin_popcount(s->fields) * ((s->flags & IBLB_AVG_SQ) ? 2 : 1) + ((s->flags & IBLB_AVG_UXUY) ? 1 : 0);
    const size_t bin = (size_t)s->planes * (size_t)s->win.nx * (size_t)s->win.ny;  // at most 21 lattices
    if ((size_t)s->nbins > (r.n / 8) / bin || !r.array(&s->bins, (size_t)s->nbins * bin) || !r.done())
        return bad(c, sec, "its length does not match its header");
    return IBLB_OK;
}

int restore_scalar(iblb_ctx* c, const CkScalar& s) {
    const ScalarGeom S = scalar_geom(c);
    const size_t ncol = (size_t)c->ncol, ny = (size_t)c->ny, N = ncol * ny;
    if ((size_t)S.plane > SIZE_MAX / sizeof(double) / 12)
        return fail(c, IBLB_ERR_NOMEM, "checkpoint: the scalar's populations exceed the address space");
    DevBuf d, in, df, dw, du, de, dg;
    HIP_TRY(c, hipMalloc(&d.p, 12 * (size_t)S.plane * sizeof(double)));
    HIP_TRY(c, hipMalloc(&in.p, 5 * N * sizeof(double)));
    double* buf = (double*)d.p;
    HIP_TRY(c, hipMemsetAsync(buf, 0, 12 * (size_t)S.plane * sizeof(double), c->stream));
    HIP_TRY(c, hipMemcpyAsync(in.p, s.pops.data(), 5 * N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, launch_scalar_in((const double*)in.p, S, 5, buf, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (s.parts & 1u) {
        HIP_TRY(c, hipMalloc(&df.p, (size_t)S.plane * sizeof(double)));
        HIP_TRY(c, hipMalloc(&dw.p, 4 * ncol * sizeof(double)));
        HIP_TRY(c, hipMemsetAsync(df.p, 0, (size_t)S.plane * sizeof(double), c->stream));
        HIP_TRY(c, hipMemcpyAsync(in.p, s.src_field.data(), N * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, launch_scalar_in((const double*)in.p, S, 1, (double*)df.p, c->stream));
        HIP_TRY(c, hipMemcpyAsync(dw.p, s.src_walls.data(), 4 * ncol * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (s.parts & 2u) {
        HIP_TRY(c, hipMalloc(&du.p, 6 * ncol * sizeof(double)));
        HIP_TRY(c, hipMemcpy(du.p, s.up.data(), 6 * ncol * sizeof(double), hipMemcpyHostToDevice));
    }
    if (s.parts & 4u) {
        HIP_TRY(c, hipMalloc(&de.p, 6 * ny * sizeof(double)));
        HIP_TRY(c, hipMemcpy(de.p, s.end.data(), 6 * ny * sizeof(double), hipMemcpyHostToDevice));
    }
    if (s.parts & 8u) {
        int rc = gauges_buffer(c, (int)s.station.size(), s.station.data(), (int)s.level.size(), s.level.data(), s.gau.data(), &dg);
        if (rc) return rc;
    }
    // everything is on the device: the context takes it
    auto take = [](DevBuf& b) {
        double* p = (double*)b.p;
        b.p = nullptr;
        return p;
    };
    c->sc_alloc = take(d);
    c->sc_g[0] = buf;
    c->sc_g[1] = buf + 5 * S.plane;
    c->sc_uv = buf + 10 * S.plane;
    c->sc_cur = 0;
    c->sc_cfg = s.cfg;
    c->sc_ev.stride = s.cfg.stride;
    c->sc_ev.count = s.events;
    c->sc_ev.next = s.t0 + (s.events + 1) * s.cfg.stride;
    if (s.parts & 1u) {
        c->sc_src_field = take(df);
        c->sc_src_walls = take(dw);
        c->sc_src_decay = s.src_decay;
        c->sc_src_present = s.src_present;
    }
    if (s.parts & 2u) {
        c->sc_up = take(du);
        c->sc_up_present = s.up_present;
        c->sc_up_substeps = s.up_substeps;
    }
    if (s.parts & 4u) {
        c->sc_end = take(de);
        for (int k = 0; k < 2; ++k) {
            c->sc_end_kind[k] = s.end_kind[k];
            c->sc_end_value[k] = s.end_value[k];
        }
        c->sc_end_present = s.end_present;
        c->sc_end_substeps = s.end_substeps;
    }
    if (s.parts & 8u) {
        c->sc_gau = take(dg);
        c->sc_gau_station = s.station;
        c->sc_gau_level = s.level;
        c->sc_gau_substeps = s.gau_substeps;
    }
    return IBLB_OK;
}

int restore_tracers(iblb_ctx* c, const CkTracers& s) {
    const size_t np = (size_t)s.n;
    DevBuf dx, dy, dl;
    HIP_TRY(c, hipMalloc(&dx.p, np * sizeof(double)));
    HIP_TRY(c, hipMalloc(&dy.p, np * sizeof(double)));
    HIP_TRY(c, hipMalloc(&dl.p, np * sizeof(int)));
    HIP_TRY(c, hipMemcpy(dx.p, s.x.data(), np * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(dy.p, s.y.data(), np * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(dl.p, s.laps.data(), np * sizeof(int), hipMemcpyHostToDevice));
    c->tr_x = (double*)dx.p;
    c->tr_y = (double*)dy.p;
    c->tr_laps = (int*)dl.p;
    dx.p = dy.p = dl.p = nullptr;
    c->tr_n = s.n;
    c->tr_ev.stride = s.stride;
    c->tr_ev.count = s.updates;
    c->tr_ev.next = s.t0 + (s.updates + 1) * s.stride;
    return IBLB_OK;
}

int restore_average(iblb_ctx* c, const CkAverage& s) {
    const size_t n = (size_t)s.planes * (size_t)s.win.nx * (size_t)s.win.ny, bytes = (size_t)s.nbins * n * sizeof(double);
    DevBuf d, in;
    HIP_TRY(c, hipMalloc(&d.p, bytes));
    HIP_TRY(c, hipMalloc(&in.p, bytes));
    HIP_TRY(c, hipMemcpyAsync(in.p, s.bins.data(), bytes, hipMemcpyHostToDevice, c->stream));
    // the readout's transpose with the window's sides exchanged is its own inverse: the ABI's planes (x fastest) back
    // into the accumulators' (y fastest)
    for (int bin = 0; bin < s.nbins; ++bin)
        HIP_TRY(c, launch_average_readout((const double*)in.p + (size_t)bin * n, s.win.ny, s.win.nx, s.planes,
                                          (double*)d.p + (size_t)bin * n, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->av_buf = (double*)d.p;
    d.p = nullptr;
    c->av_win = s.win;
    c->av_fields = s.fields;
    c->av_flags = s.flags;
    c->av_nbins = s.nbins;
    c->av_planes = s.planes;
    c->av_ev.stride = s.stride;
    c->av_ev.count = s.samples;
    c->av_ev.next = s.t0 + (s.samples + 1) * s.stride;
    c->av_count = s.count;
    return IBLB_OK;
}

}  // namespace

bool observer_set(const iblb_ctx* c, int kind) {
    return kind == iblbck::K_SCALAR ? c->sc_alloc != nullptr : kind == iblbck::K_TRACERS ? c->tr_n > 0 : c->av_fields != 0;
}

int observer_pack(iblb_ctx* c, int kind, std::vector<char>* out) {
    out->clear();
    const Put w{out};
    return kind == iblbck::K_SCALAR ? pack_scalar(c, w) : kind == iblbck::K_TRACERS ? pack_tracers(c, w) : pack_average(c, w);
}

int observers_parse(iblb_ctx* c, long long t, std::vector<char> payload[3], const bool has[3], CkObservers* o) {
    int rc = IBLB_OK;
    for (int k = 0; k < 3 && !rc; ++k) {
        o->has[k] = has[k];
        if (!has[k]) continue;
        const Get r{payload[k].data(), payload[k].size()};
        rc = k == iblbck::K_SCALAR ? parse_scalar(c, t, r, &o->sc)
             : k == iblbck::K_TRACERS ? parse_tracers(c, t, r, &o->tr)
                                      : parse_average(c, t, r, has[iblbck::K_SCALAR], &o->av);
        std::vector<char>().swap(payload[k]);
    }
    return rc;
}

int observers_restore(iblb_ctx* c, const CkObservers& o) {
    scalar_free(c);
    tracers_free(c);
    average_free(c);
    int rc = IBLB_OK;
    if (o.has[iblbck::K_SCALAR]) rc = restore_scalar(c, o.sc);
    if (!rc && o.has[iblbck::K_TRACERS]) rc = restore_tracers(c, o.tr);
    if (!rc && o.has[iblbck::K_AVERAGE]) rc = restore_average(c, o.av);
    if (rc) {
        scalar_free(c);
        tracers_free(c);
        average_free(c);
    }
    return rc;
}

}  // namespace iblbh
