// ctx_observe.hip — the observers of a context (ctx.h): what iblb_step runs between the pieces of a call
// with the state held fixed.  Passive tracers (iblb_set_tracers), time- and phase-averaged fields
// (iblb_set_average) and the passive scalar (iblb_set_scalar), each on a Periodic schedule; iblb_step asks
// next_event where to cut a call and run_events to run what is due there.  Built from the read scaffold of
// ctx.h like the readers.
#include <algorithm>
#include <cmath>
#include <vector>

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

void tracers_free(iblb_ctx* c) {
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

static size_t average_bin_elems(const iblb_ctx* c) {
    return (size_t)c->av_planes * (size_t)c->av_win.nx * (size_t)c->av_win.ny;
}

// One update of the tracers from the current state, on the context's stream: the state prepared as
// for a reader (the band streams joined, the owed IB force evaluated), then one launch.
static int tracer_update(iblb_ctx* c) {
    int rc = band_join(c);
    if (rc || (rc = prepare_read(c))) return rc;
    const FieldsArgs a = point_args(c, IBLB_FIELD_UX | IBLB_FIELD_UY);
    HIP_TRY(c, with_state(c, [&](auto* g, auto H) {
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

long long next_event(const iblb_ctx* c) {
    long long next = LLONG_MAX;
    if (c->tr_n > 0) next = std::min(next, c->tr_ev.next);
    if (c->av_fields) next = std::min(next, c->av_ev.next);
    if (c->sc_alloc) next = std::min(next, c->sc_ev.next);
    return next;
}

// No observer changes the fluid state, but an average may sample the scalar: the scalar's event runs first, so
// that a sample at a common iteration sees C after that iteration's event (include/iblb.h)
int run_events(iblb_ctx* c) {
    int rc = IBLB_OK;
    if (c->sc_alloc && c->t == c->sc_ev.next && (rc = scalar_update(c))) return rc;
    if (c->tr_n > 0 && c->t == c->tr_ev.next && (rc = tracer_update(c))) return rc;
    if (c->av_fields && c->t == c->av_ev.next) rc = average_update(c);
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
    // the index arrays of ScalarGauges: {own, the left neighbour's} per column, {own, the row below's} per row
    std::vector<int> col(2 * (size_t)ncol, -1), row(2 * (size_t)ny, -1);
    for (int k = 0; k < ga->n_stations; ++k) {
        const int x = ga->station[k];
        col[2 * (size_t)x] = k;
        col[2 * (size_t)(x + 1 < ncol ? x + 1 : 0) + 1] = k;
    }
    for (int k = 0; k < ga->n_levels; ++k) {
        const int y = ga->level[k];
        row[2 * (size_t)y] = k;
        row[2 * (size_t)(y + 1) + 1] = k;
    }
    // the new buffer first: a failed allocation leaves the previous gauges as they were
    const size_t nt = 2 * ((size_t)ga->n_stations * ny + (size_t)ga->n_levels * ncol);
    const size_t nb = nt * sizeof(double) + 2 * ((size_t)ncol + ny) * sizeof(int);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, nb));
    int* idx = (int*)((double*)d.p + nt);
    HIP_TRY(c, hipMemsetAsync(d.p, 0, nt * sizeof(double), c->stream));
    HIP_TRY(c, hipMemcpyAsync(idx, col.data(), col.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(idx + col.size(), row.data(), row.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
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
