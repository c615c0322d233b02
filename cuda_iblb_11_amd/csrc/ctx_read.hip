// ctx_read.hip — the readers of a context (ctx.h): the current state to the host in the reference
// layouts, windowed fields and reductions, point sampling and the output gather.  Every reader checks its
// arguments, prepares the state (ctx_step.hip:prepare_read), launches through with_state and ends in
// read_back (the read scaffold of ctx.h).
#include <cmath>

#include "ctx.h"

namespace iblbh {

// rho [N] and u [2N] of the slab in the reference layout (j = y*ncol + xc), into device buffers,
// on the context's stream.  The state must be prepared (prepare_read).
static int macro_device(iblb_ctx* c, double* dr, double* du) {
    if (c->phase == PH_BOOT) {
        HIP_TRY(c, launch_field_out(c->rho0, dr, c->L, 1, c->fplane, 0., 0., c->stream));
        HIP_TRY(c, launch_field_out(c->u0, du, c->L, 2, c->fplane, 0., 0., c->stream));
        return IBLB_OK;
    }
    HIP_TRY(c, with_state(c, [&](auto* g, auto H) {
        return launch_macro_out(g, c->L, H, ib_force(c), c->fplane, c->coef.gx, c->coef.gy, dr, du, c->stream);
    }));
    return IBLB_OK;
}

// The window (NULL: the whole lattice at stride 1) checked against the lattice, and the samples whose
// column this slab owns: [*i_first, *i_first + *nxl) of the window's nx.
int window_part(iblb_ctx* c, const iblb_window* w, iblb_window* win, int* i_first, int* nxl) {
    *win = w ? *w : iblb_window{0, 0, c->nx, c->ny, 1, 1};
    if (win->sx < 1 || win->sy < 1 || win->nx < 1 || win->ny < 1 || win->x0 < 0 || win->y0 < 0 ||
        (long long)win->x0 + (long long)(win->nx - 1) * win->sx >= c->nx ||
        (long long)win->y0 + (long long)(win->ny - 1) * win->sy >= c->ny)
        return fail(c, IBLB_ERR_ARG, "window: need sx, sy, nx, ny >= 1 and every sample inside the lattice (no wrap)");
    // first sample at or right of x_begin, first sample at or right of the slab's end
    auto first_at = [&](long long x) {
        const long long i = x <= win->x0 ? 0 : (x - win->x0 + win->sx - 1) / win->sx;
        return (int)std::min(i, (long long)win->nx);
    };
    const int lo = first_at(c->x_begin), hi = first_at((long long)c->x_begin + c->ncol);
    *i_first = lo;
    *nxl = hi - lo;
    return IBLB_OK;
}

// The arguments of the windowed kernels for this slab's part of window win: samples [lo, lo + nxl)
FieldsArgs window_args(iblb_ctx* c, const iblb_window& win, int lo, int nxl, unsigned fields) {
    FieldsArgs a{};
    a.xl0 = win.x0 + lo * win.sx - c->x_begin;
    a.sx = win.sx;
    a.nxl = nxl;
    a.y0 = win.y0;
    a.sy = win.sy;
    a.nyw = win.ny;
    a.fields = fields;
    a.fplane = c->fplane;
    a.gx = c->coef.gx;
    a.gy = c->coef.gy;
    a.kvisc = -c->coef.kguo;
    if (c->phase == PH_BOOT) {
        a.rho0 = c->rho0;
        a.u0 = c->u0;
    } else {
        a.fdense = ib_force(c);
    }
    if (fields & IBLB_FIELD_SCALAR) {  // (the callers checked that a scalar is set: check_scalar_fields)
        a.sc = c->sc_g[c->sc_cur];
        a.sc_rows = c->L.rows;
        a.sc_plane = (long)c->ncol * c->L.rows;
    }
    return a;
}

// Every position finite and inside [0, XDIM) x [0, YDIM-1]: the kernels index the lattice from them
int check_positions(iblb_ctx* c, long long n, const double* x, const double* y) {
    if (c->ny < 2) return fail(c, IBLB_ERR_ARG, "bilinear sampling needs YDIM >= 2");
    const double X = (double)c->nx, ytop = (double)(c->ny - 1);
    for (long long p = 0; p < n; ++p)
        if (!(std::isfinite(x[p]) && std::isfinite(y[p]) && x[p] >= 0. && x[p] < X && y[p] >= 0. && y[p] <= ytop))
            return fail(c, IBLB_ERR_ARG,
                        "point " + std::to_string(p) + " is non-finite or outside 0 <= x < XDIM, 0 <= y <= YDIM-1");
    return IBLB_OK;
}

int group_refused(iblb_ctx* c, const char* what) {
    return fail(c, IBLB_ERR_UNSUPPORTED,
                std::string(what) + ": a lone slab only (the four cells of a point may straddle the slabs of a group)");
}

}  // namespace iblbh

using namespace iblbh;

extern "C" {

int iblb_get_lagrangian(iblb_ctx* c, float* s, float* u_s, int* epsilon) {
    if (!c) return IBLB_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t ns = (size_t)c->ns;
    return read_back(c, {{s, pts_s(c), 2 * ns * sizeof(float)},
                         {u_s, pts_us(c), 2 * ns * sizeof(float)},
                         {epsilon, pts_eps(c), ns * sizeof(int)}});
}

int iblb_get_macro(iblb_ctx* c, double* rho, double* u) {
    if (!c) return IBLB_ERR_ARG;
    int rc = prepare_read(c);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const long N = (long)c->ncol * c->ny;
    const size_t nb = (size_t)N * sizeof(double);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, 3 * nb));
    if ((rc = macro_device(c, (double*)d.p, (double*)d.p + N))) return rc;
    return read_back(c, {{rho, d.p, nb}, {u, (double*)d.p + N, 2 * nb}});
}

int iblb_get_populations(iblb_ctx* c, double* f) {
    if (!c || !f) return IBLB_ERR_ARG;
    int rc = prepare_read(c);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nb = 9 * (size_t)c->ncol * c->ny * sizeof(double);
    DevBuf df;
    HIP_TRY(c, hipMalloc(&df.p, nb));
    const int raw = c->phase == PH_BOOT;  // f^0 is stored unstreamed
    HIP_TRY(c, with_state(c, [&](auto* g, auto H) { return launch_pop_out(g, c->L, H, (double*)df.p, raw, c->stream); }));
    return read_back(c, f, df.p, nb);
}

int iblb_get_force(iblb_ctx* c, double* force) {
    if (!c || !force) return IBLB_ERR_ARG;
    int rc = prepare_read(c);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nb = 2 * (size_t)c->ncol * c->ny * sizeof(double);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, nb));
    HIP_TRY(c, launch_field_out(c->phase == PH_BOOT ? c->force0 : ib_force(c), (double*)d.p, c->L, 2, c->fplane,
                                c->coef.gx, c->coef.gy, c->stream));
    return read_back(c, force, d.p, nb);
}

int iblb_get_lagrangian_force(iblb_ctx* c, float* F_s) {
    if (!c || !F_s) return IBLB_ERR_ARG;
    int rc = prepare_read(c);
    if (rc) return rc;
    if (c->ns == 0) return IBLB_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // in a group each point's F_s is held by one slab, zeros elsewhere: sum exactly
    if ((rc = group_sum(c, c->d_Fs, c->d_Fs_sum, 2 * (size_t)c->ns, ncclFloat32))) return rc;
    return read_back(c, F_s, rccl_multi(c) ? c->d_Fs_sum : c->d_Fs, 2 * (size_t)c->ns * sizeof(float));
}

int iblb_get_flux(iblb_ctx* c, double* Q) {
    if (!c || !Q) return IBLB_ERR_ARG;
    int rc = prepare_read(c);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // d_Q[1] = d_Q[0] + q(u^t) of the current (not yet collided) state
    HIP_TRY(c, hipMemcpyAsync(c->d_Q + 1, c->d_Q, sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    const int fc = c->cfg.flux_column - c->x_begin;
    if (c->phase == PH_RUN && fc >= 0 && fc < c->ncol)
        HIP_TRY(c, with_state(c, [&](auto* g, auto H) {
            return launch_flux(g, c->L, H, ib_force(c), c->fplane, c->coef.gx, c->coef.gy, fc, c->cfg.flux_norm,
                               c->d_Q + 1, c->stream);
        }));
    if ((rc = group_sum(c, c->d_Q + 1, c->d_Q + 1, 1, ncclFloat64))) return rc;
    return read_back(c, Q, c->d_Q + 1, sizeof(double));
}

int iblb_count_nonfinite(iblb_ctx* c, long long* count) {
    if (!c || !count) return IBLB_ERR_ARG;
    int rc = check_ready(c);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = band_join(c)) || (rc = join_comm(c))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->d_Q + 1, 0, sizeof(double), c->stream));
    HIP_TRY(c, with_state(c, [&](auto* g, auto) { return launch_count_nonfinite(g, c->L, c->d_Q + 1, c->stream); }));
    if ((rc = group_sum(c, c->d_Q + 1, c->d_Q + 1, 1, ncclFloat64))) return rc;
    double n = 0.;
    if ((rc = read_back(c, &n, c->d_Q + 1, sizeof(double)))) return rc;
    *count = (long long)n;
    return IBLB_OK;
}

// ---- windowed field readback ----------------------------------------------------------------------
int iblb_window_local(iblb_ctx* c, const iblb_window* w, int* i_first, int* nx_local) {
    if (!c) return IBLB_ERR_ARG;
    iblb_window win;
    int lo = 0, n = 0;
    int rc = window_part(c, w, &win, &lo, &n);
    if (rc) return rc;
    if (i_first) *i_first = lo;
    if (nx_local) *nx_local = n;
    return IBLB_OK;
}

int iblb_get_fields(iblb_ctx* c, const iblb_window* w, unsigned fields, double* out) {
    if (!c) return IBLB_ERR_ARG;
    int rc = check_fields(c, fields);
    if (rc) return rc;
    iblb_window win;
    int lo = 0, nxl = 0;
    if ((rc = window_part(c, w, &win, &lo, &nxl))) return rc;
    if (nxl > 0 && !out) return fail(c, IBLB_ERR_ARG, "out is NULL");
    if ((rc = check_vorticity(c, fields)) || (rc = check_scalar_fields(c, fields)) || (rc = prepare_read(c))) return rc;
    if (nxl == 0) return IBLB_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int nf = __builtin_popcount(fields);
    const size_t nb = (size_t)nf * win.ny * nxl * sizeof(double);
    const FieldsArgs a = window_args(c, win, lo, nxl, fields);
    DevBuf d;
    HIP_TRY(c, hipMalloc(&d.p, nb));
    HIP_TRY(c, with_state(c, [&](auto* g, auto H) { return launch_fields_out(g, c->L, H, a, (double*)d.p, c->stream); }));
    return read_back(c, out, d.p, nb);
}

// ---- window reduction ---------------------------------------------------------------------------------
int iblb_reduce_fields(iblb_ctx* c, const iblb_window* w, unsigned fields, iblb_field_stats* stats, double* row_sum,
                       double* col_sum) {
    if (!c) return IBLB_ERR_ARG;
    int rc = check_fields(c, fields, IBLB_FIELD_ALL | IBLB_QTY_ALL | IBLB_FIELD_SCALAR);
    if (rc) return rc;
    iblb_window win;
    int lo = 0, nxl = 0;
    if ((rc = window_part(c, w, &win, &lo, &nxl))) return rc;
    if (!stats) return fail(c, IBLB_ERR_ARG, "stats is NULL");
    if ((rc = check_vorticity(c, fields)) || (rc = check_scalar_fields(c, fields)) || (rc = prepare_read(c))) return rc;
    const int nf = __builtin_popcount(fields);
    if (nxl == 0) {  // none of the window's columns is this slab's
        for (int k = 0; k < nf; ++k)
            stats[k] = iblb_field_stats{0, 0, 0., 0., HUGE_VAL, -HUGE_VAL, -1, -1, -1, -1};
        if (row_sum) std::fill(row_sum, row_sum + (size_t)nf * win.ny, 0.);
        return IBLB_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    ReduceGeom q = reduce_geometry(nxl, win.ny, nf, row_sum != nullptr, col_sum != nullptr);
    q.i_first = lo;
    if ((size_t)q.n_scratch > c->red_cap) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (c->red_buf) HIP_TRY(c, hipFree(c->red_buf));
        c->red_buf = nullptr;
        c->red_cap = 0;
        if (hipMalloc((void**)&c->red_buf, (size_t)q.n_scratch * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, IBLB_ERR_NOMEM, "iblb_reduce_fields: scratch allocation failed");
        }
        c->red_cap = (size_t)q.n_scratch;
    }
    const FieldsArgs a = window_args(c, win, lo, nxl, fields);
    HIP_TRY(c, with_state(c, [&](auto* g, auto H) { return launch_reduce_fields(g, c->L, H, a, q, c->red_buf, c->stream); }));
    c->red_host.resize((size_t)q.n_out);
    if ((rc = read_back(c, c->red_host.data(), c->red_buf + q.o_out, (size_t)q.n_out * sizeof(double)))) return rc;
    const double* h = c->red_host.data();
    for (int k = 0; k < nf; ++k) {
        const double* r = h + (size_t)k * REDUCE_RS;
        stats[k] = iblb_field_stats{(long long)r[0], (long long)r[1], r[2], r[3], r[4], r[5],
                                    (int)r[6], (int)r[7], (int)r[8], (int)r[9]};
    }
    h += (size_t)nf * REDUCE_RS;
    if (row_sum) {
        std::copy(h, h + (size_t)nf * win.ny, row_sum);
        h += (size_t)nf * win.ny;
    }
    if (col_sum) std::copy(h, h + (size_t)nf * nxl, col_sum);
    return IBLB_OK;
}

// ---- point sampling -----------------------------------------------------------------------------------
int iblb_sample_points(iblb_ctx* c, int n, const double* x, const double* y, unsigned fields, double* out) {
    if (!c) return IBLB_ERR_ARG;
    if (n < 0) return fail(c, IBLB_ERR_ARG, "n is negative");
    if (n > 0 && (!x || !y || !out)) return fail(c, IBLB_ERR_ARG, "x, y or out is NULL");
    int rc = check_fields(c, fields);
    if (rc) return rc;
    if (!single_slab(c)) return group_refused(c, "iblb_sample_points");
    if ((rc = check_positions(c, n, x, y)) || (rc = check_scalar_fields(c, fields))) return rc;
    if (n == 0) return IBLB_OK;
    if ((rc = prepare_read(c))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const int nf = __builtin_popcount(fields);
    const size_t np = (size_t)n;
    std::vector<double> xy(2 * np);  // one copy in: x then y
    std::copy(x, x + np, xy.begin());
    std::copy(y, y + np, xy.begin() + np);
    DevBuf d_xy, d_out;
    HIP_TRY(c, hipMalloc(&d_xy.p, 2 * np * sizeof(double)));
    HIP_TRY(c, hipMalloc(&d_out.p, nf * np * sizeof(double)));
    HIP_TRY(c, hipMemcpyAsync(d_xy.p, xy.data(), 2 * np * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const FieldsArgs a = point_args(c, fields);
    HIP_TRY(c, with_state(c, [&](auto* g, auto H) {
        return launch_sample_points(g, c->L, H, a, (long)n, (const double*)d_xy.p, (double*)d_out.p, c->stream);
    }));
    return read_back(c, out, d_out.p, nf * np * sizeof(double));
}

// ---- output gather (RCCL group) -----------------------------------------------------------------
int iblb_gather_macro(iblb_ctx* c, int root, double* rho, double* u) {
    if (!c) return IBLB_ERR_ARG;
    if (c->transport == TR_LOCAL) return fail(c, IBLB_ERR_STATE, "local group: gather the slabs' iblb_get_macro");
    if (!rccl_multi(c)) return iblb_get_macro(c, rho, u);
    if (root < 0 || root >= c->nranks) return fail(c, IBLB_ERR_ARG, "root rank out of range");
    int rc = prepare_read(c);
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const long N = (long)c->ncol * c->ny;
    DevBuf mine, all;
    HIP_TRY(c, hipMalloc(&mine.p, 3 * (size_t)N * sizeof(double)));
    if ((rc = macro_device(c, (double*)mine.p, (double*)mine.p + N))) return rc;
    const bool is_root = c->rank == root;
    const size_t total = 3 * (size_t)c->nx * c->ny;
    if (is_root) HIP_TRY(c, hipMalloc(&all.p, total * sizeof(double)));
    if ((rc = rccl_order(c, c->stream))) return rc;
    // rank r's [rho | u] block lands at 3*ny*x_begin_r in rank order
    NCCL_TRY(c, ncclGroupStart());
    if (is_root) {
        for (int r = 0; r < c->nranks; ++r) {
            double* dst = (double*)all.p + 3L * c->ny * c->slab_begin[r];
            const size_t n = 3 * (size_t)c->ny * c->slab_count[r];
            if (r == root) HIP_TRY(c, hipMemcpyAsync(dst, mine.p, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            else NCCL_TRY(c, ncclRecv(dst, n, ncclFloat64, r, c->comm, c->stream));
        }
    } else {
        NCCL_TRY(c, ncclSend(mine.p, 3 * (size_t)N, ncclFloat64, root, c->comm, c->stream));
    }
    NCCL_TRY(c, ncclGroupEnd());
    std::vector<double> h(is_root && (rho || u) ? total : 0);  // (the others only synchronise)
    if ((rc = read_back(c, h.data(), all.p, h.size() * sizeof(double))) || h.empty()) return rc;
    const long nx = c->nx, ny = c->ny, G = nx * ny;
    for (int r = 0; r < c->nranks; ++r) {
        const long xb = c->slab_begin[r], nc = c->slab_count[r], n = nc * ny;
        const double* blk = h.data() + 3 * ny * xb;
        for (long y = 0; y < ny; ++y)
            for (long xc = 0; xc < nc; ++xc) {
                const long j = y * nc + xc, g = y * nx + xb + xc;
                if (rho) rho[g] = blk[j];
                if (u) {
                    u[g] = blk[n + j];
                    u[G + g] = blk[2 * n + j];
                }
            }
    }
    return IBLB_OK;
}

}  // extern "C"
