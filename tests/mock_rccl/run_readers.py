#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: every reader of the C ABI on the slabs of an RCCL group, in the middle of a
run, between deep slab cycles, IB band cycles and per-iteration steps.  N ranks run as threads on one
GPU through the mock-RCCL build (tests/mock_rccl/libiblb_mockrccl.so), beside a lone-slab twin of the
same build that takes the same state.  Prints one JSON line; exit status 0 = pass.

usage: run_readers.py NRANKS NX NY MODE PRECISION(f64/f32) [ROTATE] [nan]

MODE  0   no IB, bulk calls 1, K, 2K, 3, K + 3 (K = IBLB_SWEEP_DEPTH): boot step, one deep cycle, two
          chained cycles, remainders, a cycle plus remainders
      0s  no IB, 12 calls of one iteration
      1   points given per iteration (set_lagrangian + step(1)): run_group.py's three filaments
      2   a schedule, one filament inside each slab, bulk calls as mode 0 (IB band cycles)
      3   a schedule, one filament across every slab edge (x = 0 included), bulk calls
nan   (mode 0) the short scenario of iblb_count_nonfinite's non-zero case instead of the run

A read point falls before the first step and after every call (bulk modes) / every third iteration
(0s, 1).  At a read point every rank calls every reader (READERS below) on every window, all ranks in
the same order; read point p starts the list at entry (p + ROTATE) mod its length, so that from one
read point to the next another reader is the call that meets the stale halo and the owed IB force.
The workers only record; everything is compared afterwards, on the main thread.  Right after the step
call of read point 2, with the halo stale, all ranks together issue the calls the header refuses
(vorticity on a slab, a window past nx, an unknown field bit, stats == NULL): each returns its code and,
with profiling on, timing()["halo_ms"] stays the same double (no exchange was issued: the check came
before anything collective); the readers that follow then do raise it.

Bounds (none of them fitted to the code under test):
  run_group.py     macro / force against the twin: bit-equal without IB, 1e-12 (f64) / 1e-5 (f32) of
                   the array's own max with IB; flux 1e-12 relative; F_s 1e-5 of its max
  test_gpu_fields  fields against fields_ref of the same rank's macro() and populations(): rho, ux, uy
                   bit-equal, stress within 64 * 2^-52 * max rho (its slab_ref / check)
  iblb.h           reduce: counts, extrema and their indices exact, every sum within
                   n * 2^-53 * sum|x| of the exact sum (reduce_ref.check); the same for the ranks' parts
                   merged by lattice.combine_stats against the whole window's samples
"""
import ctypes as C
import json
import math
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p_ in (TESTS, os.path.dirname(TESTS)):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

BULK_MODES = ("0", "2", "3")
IB_MODES = ("1", "2", "3")
READERS = ["macro", "populations", "force", "flux", "count_nonfinite", "lagrangian_force", "fields", "reduce",
           "window_local", "gather_macro"]
LOCAL = ["rho", "ux", "uy", "sxx", "sxy", "syy"]
REDUCED = LOCAL + ["momx", "momy", "ke", "usq"]


def reader_order(ib, p, last, rotate):
    """The readers of read point p in calling order: lagrangian_force in IB modes only, gather_macro
    at the last read point only; the list starts at entry (p + rotate) mod its length."""
    names = [n for n in READERS if (ib or n != "lagrangian_force") and (last or n != "gather_macro")]
    k = (p + rotate) % len(names)
    return names[k:] + names[:k]


def first_reader(ib, p, last, rotate):
    """The first collective reader of read point p (iblb_window_local touches no halo)."""
    return [n for n in reader_order(ib, p, last, rotate) if n != "window_local"][0]


def read_points(mode, K):
    """(calls, iterations after which a read point falls): read point 0 is before the first step."""
    if mode in BULK_MODES:
        calls = [1, K, 2 * K, 3, K + 3]
        return calls, list(np.cumsum(calls))
    return [1] * 12, [3, 6, 9, 12]


def windows(nx, ny, slabs):
    xb1, xc1 = slabs[1]
    return [None,
            (1, 1, (nx - 2) // 3 + 1, (ny - 2) // 2 + 1, 3, 2),
            (xb1 + xc1 // 2 - 2, 2, 3, 4, 2, 3),  # three columns inside slab 1: nx_local == 0 elsewhere
            (xb1 - 1, 0, 2, ny, 1, 1),            # the last column of slab 0 and the first of slab 1
            (nx - 1, 0, 1, ny, 1, 1),
            (0, ny - 1, nx, 1, 1, 1)]


failures = []
errors = []


def fail(*what):
    if len(failures) < 40:
        failures.append(" ".join(str(w) for w in what))


def guarded(fn):
    def run(r):
        try:
            fn(r)
        except Exception as e:  # a failed rank would leave the others waiting: report and exit hard
            errors.append(f"rank {r}: {e!r}")
            print(json.dumps({"ok": False, "errors": errors}), flush=True)
            os._exit(2)
    return run


def run_ranks(fn, n):
    th = [threading.Thread(target=fn, args=(r,)) for r in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join()


class Cached:
    """What test_gpu_fields.slab_ref asks of a slab, answered from one read point's record (no
    further collective calls)."""

    def __init__(self, nx, ny, xb, xc, rec):
        self.nx, self.ny, self.x_begin, self.x_count, self._rec = nx, ny, xb, xc, rec

    def macro(self):
        return self._rec["macro"]

    def populations(self):
        return self._rec["populations"]


def main():
    from cuda_iblb_11_amd import _lib as L
    from cuda_iblb_11_amd import workloads as W
    from cuda_iblb_11_amd.lattice import (Lattice, combine_stats, plan_slabs, rccl_unique_id, split_populations,
                                          split_state)
    import reduce_ref as RR
    from test_gpu_fields import EPS, check as fields_check, slab_ref

    n, nx, ny, mode, prec = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    extra = sys.argv[6:]
    nan_case = "nan" in extra
    rotate = ([int(a) for a in extra if a.lstrip("-").isdigit()] or [0])[0]
    if mode not in ("0", "0s", "1", "2", "3") or n < 2 or (nan_case and mode != "0"):
        sys.exit(__doc__)
    ib = mode in IB_MODES
    K = int(os.environ.get("IBLB_SWEEP_DEPTH", "5"))
    overlap = os.environ.get("IBLB_OVERLAP", "1") != "0"
    lib = L.load_from(os.path.join(HERE, "libiblb_mockrccl.so"))
    slabs = plan_slabs(nx, n)
    rho, u = W.perturbed_state(nx, ny, 31)
    bf = (1e-6, 2e-7)
    fcol = nx - 5
    mp = 96 if ib else 0
    kw = dict(precision=prec, body_force=bf, max_points=mp, lib=lib, flux_column=fcol)
    if nan_case:
        return nan_scenario(n, nx, ny, slabs, rho, u, kw)

    # ---- points (run_group.py's generators) -----------------------------------------------------
    edge = slabs[0][1] - 0.4  # filament straddling the slab 0 | slab 1 edge
    mid = slabs[0][1] / 2 + 0.2  # inner points of slab 0 (IB without the halo)

    def pts(it):  # plus one at x = XDIM (nodes wrap to column 0 of the next row)
        a = W.filament(it, n_points=40, x0=edge, y0=1.0, U0=2e-3, period=30, sway=2.0)
        b = W.filament(it, n_points=20, x0=nx - 0.3, y0=50.0, U0=2e-3, period=30, sway=0.5)
        c = W.filament(it, n_points=16, x0=mid, y0=80.0, U0=2e-3, period=30, sway=1.0)
        return tuple(np.concatenate([p, q, r]) for p, q, r in zip(a, b, c))
    if mode == "2":
        def pts(it):
            parts = []
            for xb_, xc_ in slabs:
                ph = 2 * np.pi * it / 20
                parts.append(W.filament(it, n_points=12, x0=xb_ + xc_ / 2 + 0.3 + np.sin(ph), y0=10.0, U0=2e-3,
                                        period=20, sway=0.8))
            return tuple(np.concatenate(q) for q in zip(*parts))
    if mode == "3":
        def pts(it):
            parts = []
            for r, (xb_, xc_) in enumerate(slabs):
                ph = 2 * np.pi * (it + 3 * r) / 20
                f = W.filament(it, n_points=12, x0=xb_ + 0.3 + 1.5 * np.sin(ph), y0=10.0 + 7 * r, U0=2e-3,
                               period=20, sway=1.2)
                f[0][0::2] = np.mod(f[0][0::2], nx)  # wrapped into [0, XDIM)
                parts.append(f)
            return tuple(np.concatenate(q) for q in zip(*parts))

    def sched(t0, k):
        e = [pts(it) for it in range(t0, t0 + k)]
        return np.stack([x[0] for x in e]), np.stack([x[1] for x in e]), np.stack([x[2] for x in e])

    calls, read_at = read_points(mode, K)
    steps = sum(calls)
    n_points = len(read_at) + 1
    wins = windows(nx, ny, slabs)

    def drive(lat, at_read_point, after_call=None):
        """The run of one context: its points, its calls, the read points."""
        if mode in ("2", "3"):
            lat.set_lagrangian_steps(*sched(0, steps))
        elif mode == "1":
            lat.set_lagrangian(*pts(0))  # the readers before the first step see the first points
        at_read_point(0)
        t = 0
        for k in calls:
            if mode == "1":
                lat.set_lagrangian(*pts(t))
            lat.step(k)
            t += k
            if t in read_at:
                p = read_at.index(t) + 1
                if after_call:
                    after_call(p)
                at_read_point(p)

    # ---- the twin: one lone slab, the same calls ---------------------------------------------------
    twin = Lattice(nx, ny, W.TAU, W.TAU2, **kw)
    twin.set_state(rho, u)
    T = [None] * n_points

    def twin_reads(p):
        T[p] = {"macro": twin.macro(), "populations": twin.populations(), "force": twin.force(), "flux": twin.flux,
                "lagrangian_force": twin.lagrangian_force() if ib else None,
                "fields": [twin.fields(LOCAL, w) for w in wins]}
    drive(twin, twin_reads)
    twin.close()

    # ---- the group ------------------------------------------------------------------------------
    uid = rccl_unique_id(lib)
    G = [[None] * n_points for _ in range(n)]
    timing = [None] * n
    halo_ms = [None] * n
    refused_at = 2  # the refused calls come right after this read point's step call (two chained cycles)

    @guarded
    def worker(r):
        xb, xc = slabs[r]
        lat = Lattice(nx, ny, W.TAU, W.TAU2, x_begin=xb, x_count=xc, **kw)
        lat.set_state(split_state(rho, 1, nx, ny, xb, xc), split_state(u, 2, nx, ny, xb, xc))
        lat.attach_rccl(uid, n, r)
        lat.set_profiling(True)
        h = lat.handle

        def refused(p):
            """Argument errors are checked before anything collective: with the halo stale, every
            refused call returns its code and no exchange is issued (halo_ms stays the same double)."""
            if p != refused_at:
                return
            before = lat.timing()["halo_ms"]
            out = np.full(8, -7.0)
            po = out.ctypes.data_as(C.c_void_p)
            st = (L.FieldStats * 2)()
            past = L.Window(nx - 1, 0, 2, 1, 1, 1)
            small = L.Window(0, 0, 2, 2, 1, 1)
            try:
                lat.fields(["vort"])
                code = L.IBLB_OK
            except L.IblbError as e:
                code = e.code
            got = {"fields vort": (code, L.IBLB_ERR_UNSUPPORTED),
                   "fields window past nx": (lib.iblb_get_fields(h, C.byref(past), 1, po), L.IBLB_ERR_ARG),
                   "reduce window past nx": (lib.iblb_reduce_fields(h, C.byref(past), 1, st, None, None), L.IBLB_ERR_ARG),
                   "fields unknown bit": (lib.iblb_get_fields(h, C.byref(small), 128, po), L.IBLB_ERR_ARG),
                   "reduce unknown bit": (lib.iblb_reduce_fields(h, C.byref(small), 2048, st, None, None), L.IBLB_ERR_ARG),
                   "reduce stats NULL": (lib.iblb_reduce_fields(h, C.byref(small), 1, None, None, None), L.IBLB_ERR_ARG)}
            after = lat.timing()["halo_ms"]
            for what, (rc, want) in got.items():
                if rc != want:
                    fail("refused call", what, "rank", r, "returned", rc, "expected", want)
            if not np.all(out == -7.0):
                fail("refused call wrote its output, rank", r)
            if before != after:
                fail("refused calls issued an exchange: halo_ms", before, "->", after, "rank", r)
            halo_ms[r] = after

        def reads(p):
            last = p == n_points - 1
            rec = {"order": reader_order(ib, p, last, rotate)}
            wi = [(p + k) % len(wins) for k in range(len(wins))]  # the windows rotate too
            for name in rec["order"]:
                if name == "macro":
                    rec[name] = lat.macro()
                elif name == "populations":
                    rec[name] = lat.populations()
                elif name == "force":
                    rec[name] = lat.force()
                elif name == "flux":
                    rec[name] = lat.flux
                elif name == "count_nonfinite":
                    rec[name] = lat.count_nonfinite()
                elif name == "lagrangian_force":
                    rec[name] = lat.lagrangian_force()
                elif name == "fields":
                    rec[name] = {k: lat.fields(LOCAL, wins[k]) for k in wi}
                elif name == "reduce":
                    rec[name] = {k: lat.reduce(REDUCED, wins[k], rows=True, cols=True) for k in wi}
                elif name == "window_local":
                    rec[name] = {k: lat.window_local(wins[k]) for k in wi}
                elif name == "gather_macro":
                    rec[name] = lat.gather_macro(0)
            G[r][p] = rec
            # the halo was stale behind the refused calls: the readers that followed did exchange it
            if p == refused_at and not lat.timing()["halo_ms"] > halo_ms[r]:
                fail("read point", p, "rank", r, "exchanged no halo: halo_ms stayed", halo_ms[r])

        drive(lat, reads, refused)
        # the end of the run, read once more: reading did not disturb the run
        G[r].append({"macro": lat.macro(), "populations": lat.populations(), "force": lat.force(), "flux": lat.flux,
                     "steps": lat.steps})
        timing[r] = lat.timing()
        lat.close()

    run_ranks(worker, n)

    # ---- the comparison ----------------------------------------------------------------------------
    tol = 1e-12 if prec == "f64" else 1e-5
    mx = {"d_macro": 0.0, "d_force": 0.0, "d_flux": 0.0, "d_F_s": 0.0, "stress_err": 0.0, "stress_bound": 0.0,
          "stress_max": 0.0, "part_sum_err_over_bound": 0.0, "combined_sum_err_over_bound": 0.0, "combined_sum_err": 0.0}
    rel = lambda a, b: float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)  # (F_s is float32)
    compared = 0

    def against_twin(rec, tw, what, r):
        """macro, populations, force and flux of one rank against the twin's columns."""
        nonlocal compared
        xb, xc = slabs[r]
        r1, u1 = tw["macro"]
        rs, us = rec["macro"]
        parts = [("rho", rs, split_state(r1, 1, nx, ny, xb, xc), r1), ("u", us, split_state(u1, 2, nx, ny, xb, xc), u1),
                 ("force", rec["force"], split_state(tw["force"], 2, nx, ny, xb, xc), tw["force"])]
        for name, got, ref, whole in parts:
            compared += got.size
            if got.shape != ref.shape:
                fail(what, name, "rank", r, "shape", got.shape, ref.shape)
                continue
            if not ib:  # same per-cell arithmetic, halos carry identical values: bit-identical
                if not np.array_equal(got, ref):
                    fail(what, name, "rank", r, "differs from the twin by", float(np.max(np.abs(got - ref))))
            else:
                d = float(np.max(np.abs(got - ref)) / max(np.max(np.abs(whole)), 1e-300))
                key = "d_force" if name == "force" else "d_macro"
                mx[key] = max(mx[key], d)
                if not d <= tol:
                    fail(what, name, "rank", r, "relative deviation", d, ">", tol)
        if not ib:
            fs = split_populations(tw["populations"], nx, ny, xb, xc)
            if not np.array_equal(rec["populations"], fs):
                fail(what, "populations rank", r, "differ from the twin by",
                     float(np.nanmax(np.abs(rec["populations"] - fs))))
        dq = abs(rec["flux"] - tw["flux"]) / max(abs(tw["flux"]), 1e-300)
        mx["d_flux"] = max(mx["d_flux"], float(dq))
        if not dq <= 1e-12:
            fail(what, "flux rank", r, rec["flux"], "twin", tw["flux"], "relative", dq)

    first_counts = {}
    for p in range(n_points):
        tw = T[p]
        for r in range(n):
            rec = G[r][p]
            xb, xc = slabs[r]
            what = f"read point {p}"
            against_twin(rec, tw, what, r)
            if rec["count_nonfinite"] != 0:
                fail(what, "count_nonfinite rank", r, rec["count_nonfinite"])
            if ib:
                fr, f1 = rec["lagrangian_force"], tw["lagrangian_force"]
                d = rel(fr, f1) if fr.shape == f1.shape and f1.size else math.inf
                mx["d_F_s"] = max(mx["d_F_s"], d)
                if not d <= 1e-5:
                    fail(what, "F_s rank", r, "relative deviation", d)
                if not np.array_equal(fr, G[0][p]["lagrangian_force"]):
                    fail(what, "F_s differs between rank 0 and rank", r)
            slab = Cached(nx, ny, xb, xc, rec)
            for k, w in enumerate(wins):
                ww = f"{what} window {k} rank {r}"
                # window_local against the brute-force enumeration of slab_ref
                ref, i_first, nxl, rho_s, u_s = slab_ref(slab, w)
                i0, n_loc = rec["window_local"][k]
                if n_loc != nxl or (nxl and i0 != i_first):
                    fail(ww, "window_local", (i0, n_loc), "expected", (i_first, nxl))
                    continue
                got = rec["fields"][k]
                if any(got[m].shape != ref[m].shape for m in LOCAL):
                    fail(ww, "fields shape", got["rho"].shape, ref["rho"].shape)
                    continue
                if not ib:  # the field_eval.h functions on identical bits
                    tf = tw["fields"][k]
                    for m in LOCAL:
                        if not np.array_equal(got[m], tf[m][:, i0:i0 + nxl]):
                            fail(ww, "field", m, "differs from the twin's")
                else:  # fields_ref of this rank's own macro() and populations()
                    if nxl:
                        mx["stress_err"] = max([mx["stress_err"]] +
                                               [float(np.max(np.abs(got[m] - ref[m]))) for m in ("sxx", "sxy", "syy")])
                        mx["stress_bound"] = EPS * float(np.max(rho_s))
                        mx["stress_max"] = max([mx["stress_max"]] + [float(np.max(np.abs(ref[m]))) for m in ("sxx", "sxy", "syy")])
                    try:
                        fields_check(got, ref, rho_s, u_s, LOCAL, ww)
                    except AssertionError as e:
                        fail("fields:", e)
                # reduce against reduce_ref of this rank's own fields() output
                red = rec["reduce"][k]
                rref = RR.reduce_ref({m: v for m, v in RR.with_derived(got).items() if m in REDUCED}, i0)
                if list(red) != REDUCED:
                    fail(ww, "reduce order", list(red))
                wny = ny if w is None else w[3]
                for m in REDUCED:
                    s = red[m]
                    try:
                        RR.check(s, rref[m], (ww, m))
                    except AssertionError as e:
                        fail("reduce:", e)
                    if rref[m].sum_bound > 0:
                        mx["part_sum_err_over_bound"] = max(mx["part_sum_err_over_bound"],
                                                            abs(s.sum - rref[m].sum) / rref[m].sum_bound)
                    if nxl == 0:  # the header's empty statistics
                        if (s.count, s.nonfinite, s.sum, s.sum_sq, s.min, s.max, s.min_i, s.min_j, s.max_i, s.max_j) != \
                                (0, 0, 0.0, 0.0, math.inf, -math.inf, -1, -1, -1, -1) or s.row_sum.shape != (wny,) or \
                                np.any(s.row_sum != 0) or s.col_sum.size != 0:
                            fail(ww, m, "nx_local == 0 but the statistics are not empty:", s)
        # over the ranks: the parts of every window are disjoint, in slab order and complete; the merged
        # statistics are those of the whole window's samples
        for k, w in enumerate(wins):
            wnx = nx if w is None else w[2]
            at = 0
            for r in range(n):
                i0, n_loc = G[r][p]["window_local"][k]
                if n_loc and i0 != at:
                    fail(f"read point {p} window {k}: rank {r} starts at sample {i0}, the ranks before it end at {at}")
                at += n_loc
            if at != wnx:
                fail(f"read point {p} window {k}: the ranks' nx_local sum to {at}, the window has {wnx}")
                continue
            cat = {m: np.concatenate([G[r][p]["fields"][k][m] for r in range(n)], axis=1) for m in LOCAL}
            whole = RR.reduce_ref({m: v for m, v in RR.with_derived(cat).items() if m in REDUCED}, 0)
            merged = combine_stats([G[r][p]["reduce"][k] for r in range(n)])
            for m in REDUCED:
                try:
                    RR.check(merged[m], whole[m], (f"read point {p} window {k} merged", m))
                except AssertionError as e:
                    fail("combine_stats:", e)
                err = abs(merged[m].sum - whole[m].sum)
                mx["combined_sum_err"] = max(mx["combined_sum_err"], err)
                if whole[m].sum_bound > 0:
                    mx["combined_sum_err_over_bound"] = max(mx["combined_sum_err_over_bound"], err / whole[m].sum_bound)
        if p > 0:  # (read point 0 is in the boot phase: no halo to be stale)
            f = first_reader(ib, p, p == n_points - 1, rotate)
            if [q for q in G[0][p]["order"] if q != "window_local"][0] != f:
                fail("read point", p, "did not start with", f)
            first_counts[f] = first_counts.get(f, 0) + 1
    # every read point after a step starts with another reader: at least three different ones in a run
    if len(first_counts) < 3:
        fail("the rotation is stuck: first readers", first_counts)

    # gather_macro(0) at the last read point: the assembled slabs on rank 0, nothing elsewhere
    last = n_points - 1
    R, U = np.empty((ny, nx)), np.empty((2, ny, nx))
    for r, (xb, xc) in enumerate(slabs):
        rs, us = G[r][last]["macro"]
        R[:, xb:xb + xc] = rs.reshape(ny, xc)
        U[:, :, xb:xb + xc] = us.reshape(2, ny, xc)
    g0 = G[0][last]["gather_macro"]
    gather_ok = bool(g0[0] is not None and np.array_equal(g0[0], R.ravel()) and np.array_equal(g0[1], U.ravel()) and
                     all(G[r][last]["gather_macro"] == (None, None) for r in range(1, n)))
    if not gather_ok:
        fail("gather_macro(0) differs from the assembled slabs, or a rank other than 0 received arrays")

    # the end of the run by the same rules, and what ran on the way
    for r in range(n):
        end = G[r][n_points]
        if end["steps"] != steps:
            fail("rank", r, "ended at iteration", end["steps"], "expected", steps)
        against_twin(end, T[last], "end of the run", r)
        tm = timing[r]
        if mode in ("2", "3") and tm["band_cycles"] < 4:
            fail("rank", r, "ran", tm["band_cycles"], "band cycles, expected >= 4")
        if mode == "0":
            if K >= 3:
                if tm["sweepk_launches"] <= 0:
                    fail("rank", r, "no deep launch was counted")
                # the device word carries the hand-off of chained cycles on two streams (the default of both
                # precisions: one way in f64, two-way in f32); IBLB_OVERLAP=0 runs a cycle in sequence on one
                # stream and waits on no device word, by design
                if overlap and tm["dev_wait_launches"] <= 0:
                    fail("rank", r, "no launch waited on the device word")
                if not overlap and tm["dev_wait_launches"] != 0:
                    fail("rank", r, "IBLB_OVERLAP=0 but", tm["dev_wait_launches"], "launches waited on the device word")
            else:  # depth 2: two-iteration sweeps with the 2-column halo, no deep launch by design
                if tm["sweep_launches"] <= 0 or tm["sweepk_launches"] != 0:
                    fail("rank", r, "depth 2: sweep launches", tm["sweep_launches"], "deep launches", tm["sweepk_launches"])
    if compared == 0:
        fail("nothing was compared")
    ok = not failures
    print(json.dumps({"ok": ok, "mode": mode, "n": n, "precision": prec, "depth": K, "rotate": rotate, "steps": steps,
                      "read_points": n_points, "first_reader_counts": first_counts, "gather_ok": gather_ok,
                      "tolerance": tol, **mx,
                      "band_cycles": [t["band_cycles"] for t in timing],
                      "sweepk_launches": [t["sweepk_launches"] for t in timing],
                      "dev_wait_launches": [t["dev_wait_launches"] for t in timing],
                      "failures": failures}), flush=True)
    sys.exit(0 if ok else 1)


def nan_scenario(n, nx, ny, slabs, rho, u, kw):
    """iblb_count_nonfinite's non-zero case on a group: NaN in three cells of slab 1 and one cell of the
    last slab, set through set_state(f=...), no steps.  Every rank reports the twin's total; reduce of
    rho on the whole lattice reports each rank's own non-finite cells."""
    from cuda_iblb_11_amd import workloads as W
    from cuda_iblb_11_amd.lattice import Lattice, rccl_unique_id, split_populations, split_state
    xb1, xc1 = slabs[1]
    cells = [(5, xb1), (64, xb1 + xc1 // 2), (ny - 1, xb1 + xc1 - 1), (0, nx - 1)]  # (y, x)
    rho = rho.copy()
    for y, x in cells:
        rho[y * nx + x] = np.nan
    per_rank = [sum(1 for _, x in cells if xb <= x < xb + xc) for xb, xc in slabs]
    twin = Lattice(nx, ny, W.TAU, W.TAU2, **kw)
    twin.set_state(rho, u)  # f^0 = the equilibrium of (rho, u): every population of a NaN cell is NaN
    f = twin.populations()
    twin.set_state(rho, u, f=f)
    total = twin.count_nonfinite()
    twin_rho = twin.reduce("rho")["rho"]
    twin.close()
    if total != 9 * len(cells):
        fail("the twin counts", total, "non-finite populations, expected", 9 * len(cells))
    if (twin_rho.nonfinite, twin_rho.count) != (len(cells), nx * ny - len(cells)):
        fail("the twin's reduce of rho:", twin_rho)
    uid = rccl_unique_id(kw["lib"])
    counts, reduced = [None] * n, [None] * n

    @guarded
    def worker(r):
        xb, xc = slabs[r]
        lat = Lattice(nx, ny, W.TAU, W.TAU2, x_begin=xb, x_count=xc, **kw)
        lat.set_state(split_state(rho, 1, nx, ny, xb, xc), split_state(u, 2, nx, ny, xb, xc),
                      f=split_populations(f, nx, ny, xb, xc))
        lat.attach_rccl(uid, n, r)
        counts[r] = lat.count_nonfinite()
        reduced[r] = lat.reduce("rho")["rho"]
        lat.close()

    run_ranks(worker, n)
    for r, (xb, xc) in enumerate(slabs):
        if counts[r] != total:
            fail("rank", r, "counts", counts[r], "non-finite populations, the twin", total)
        if (reduced[r].nonfinite, reduced[r].count) != (per_rank[r], xc * ny - per_rank[r]):
            fail("rank", r, "reduce of rho:", reduced[r], "expected non-finite", per_rank[r])
    ok = not failures
    print(json.dumps({"ok": ok, "mode": "0 nan", "n": n, "precision": kw["precision"], "twin_count": total,
                      "counts": counts, "rho_nonfinite": [s.nonfinite for s in reduced], "expected": per_rank,
                      "failures": failures}), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
