"""The IB band paths at the walls, in the lattice corners, on odd heights and under points that change
rows (inputs: tests/ib_edges.py), against the oracle.

Bounds.  f64 fields (rho - 1, u_x, u_y, each over its own maximum): 2x how far the oracle drifts from
itself on the same input under per-iteration population perturbations of 2^-52 .. 2^-48
(tests/golden/ib_edge_envelope.json, pinned by tests/test_oracle.py::test_ib_edge_envelope; the rule of
test_gpu_fused.py::test_ib_band_many_points) — never measured from the GPU; F_s within 2x the
envelope's float ulps.  f32: the north star 1e-4.  force, flux and the arrangements against each other:
the bounds of test_gpu_fused.py's band tests.  Every case prints the figures it asserts (pytest -s).
The step counts are the envelope's, built from the library's default deep-sweep depth K = 7.
"""
import contextlib
import json
import os

import numpy as np
import pytest

import ib_edges as E
import ib_flips

pytestmark = pytest.mark.gpu

TOL32 = 1e-4
K = E.K
ENV = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "ib_edge_envelope.json")))["configs"]
BODY = (1e-6, 0.0)
KNOBS = ("IBLB_BAND_MERGE", "IBLB_BAND_PAR", "IBLB_BAND_VHALF", "IBLB_IB_BAND")
ARRANGEMENTS = {"default": {}, "chained-serial": {"IBLB_BAND_MERGE": "0", "IBLB_BAND_PAR": "0"}}


@contextlib.contextmanager
def _knobs(**kv):
    """The band knobs of one run (read when the lattice is created and planned); everything else unset."""
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (m if m > 0 else 1.0))


def fields_rel(rho, u, rho_ref, u_ref):
    n = rho.size
    return {"rho-1": rel(rho - 1, rho_ref - 1), "ux": rel(u[:n], u_ref[:n]), "uy": rel(u[n:], u_ref[n:])}


def _against(ref, lat, precision, field_bound, ulp_bound, what, *, fs=True, flux=True):
    """Fields, force, F_s and flux of lat against an oracle snapshot; returns the figures."""
    f64 = precision == "f64"
    rho, u = lat.macro()
    out = dict(fields_rel(rho, u, ref["rho"], ref["u"]), force=rel(lat.force(), ref["force"]))
    if fs:
        got = lat.lagrangian_force()
        out["fs_ulps"] = int(ib_flips.float_ulps(got, ref["F_s"]).max())
        out["fs_rel"] = rel(got, ref["F_s"])
    if flux:
        out["flux"] = abs(lat.flux - ref["flux"]) / max(abs(ref["flux"]), 1e-30)
    print(json.dumps({"case": what, "precision": precision, "field_bound": field_bound if f64 else TOL32,
                      "fs_ulp_bound": ulp_bound if f64 else None, **out}), flush=True)
    assert max(out["rho-1"], out["ux"], out["uy"]) <= (field_bound if f64 else TOL32), (what, out)
    assert out["force"] <= (1e-9 if f64 else 1e-3), (what, out)
    if fs:
        assert (out["fs_ulps"] <= ulp_bound) if f64 else (out["fs_rel"] <= 1e-2), (what, out)
    if flux:
        assert out["flux"] <= (1e-9 if f64 else 1e-4), (what, out)
    return out


def _snapshot(sim):
    return {"rho": sim.rho.copy(), "u": sim.u.copy(), "force": sim.force.copy(), "F_s": sim.F_s.copy(),
            "flux": sim.flux}


# ---- static points on the walls and in the corners ---------------------------------------------------
_static_ref, _static_runs = {}, {}


def _static_reference(O, ny):
    """The oracle after STATIC_STEPS iterations, computed once per height."""
    if ny not in _static_ref:
        from cuda_iblb_11_amd import workloads as W
        rho, u = W.perturbed_state(E.NX, ny, E.STATE_SEED[ny])
        sim = O.Simulation(E.NX, ny, W.TAU, W.TAU2, rho=rho, u=u, body_force=BODY)
        sim.set_lagrangian(*E.wall_points(E.NX, ny))
        sim.step(E.STATIC_STEPS)
        _static_ref[ny] = _snapshot(sim)
    return _static_ref[ny]


def _static_run(P, O, precision, ny, name, **knobs):
    """One GPU run of the static configuration under the given knobs, checked against the oracle; run once
    per (precision, ny, name) and kept for the comparisons between arrangements."""
    key = (precision, ny, name)
    if key in _static_runs:
        return _static_runs[key]
    from cuda_iblb_11_amd import workloads as W
    ref = _static_reference(O, ny)
    env = ENV[f"static_{E.NX}x{ny}"]
    assert env["config"]["steps"] == E.STATIC_STEPS
    rho, u = W.perturbed_state(E.NX, ny, E.STATE_SEED[ny])
    with _knobs(**knobs):
        lat = P.Lattice(E.NX, ny, W.TAU, W.TAU2, precision=precision, body_force=BODY, max_points=4096)
        try:
            lat.set_state(rho, u)
            lat.set_lagrangian(*E.wall_points(E.NX, ny))
            lat.set_profiling(True)
            first = None
            for n in (1, 2 * K + 2, K, 3 * K):  # boot, 2 + 1 + 3 band cycles, two one-step remainders
                lat.step(n)
                lat.macro()
                lat.force()
                if n == 2 * K + 2:  # (a process's first cycles carry the kernels' first-use cost: timed apart)
                    first = lat.timing(reset=True)
            assert lat.steps == E.STATIC_STEPS
            tm = lat.timing()  # ib_ms: of the last four cycles; the counters: of the whole run
            for k in ("band_cycles", "band_merged_cycles", "band_par_cycles", "sweepk_launches", "fused_cells"):
                tm[k] += first[k]
            print(json.dumps({"case": f"static {ny} {name}", "precision": precision,
                              **{k: tm[k] for k in ("band_cycles", "band_merged_cycles", "band_par_cycles",
                                                    "sweepk_launches", "fused_cells", "ib_ms")}}), flush=True)
            errs = _against(ref, lat, precision, 2 * env["max_fields"], 2 * env["max_fs_ulps"], f"static {ny} {name}")
            _static_runs[key] = {"macro": lat.macro(), "flux": lat.flux, "tm": tm, "errs": errs}
        finally:
            lat.close()
    return _static_runs[key]


def _agree(a, b, tol, what):
    (r1, u1), (r0, u0) = a["macro"], b["macro"]
    d = (rel(r1, r0), rel(u1, u0))
    print(json.dumps({"case": what, "rho": d[0], "u": d[1], "bounds": list(tol)}), flush=True)
    assert d[0] <= tol[0] and d[1] <= tol[1], (what, d)
    if "flux" in a and "flux" in b:  # (the looser of the two tolerances: 1e-11 in f64, 1e-5 in f32)
        assert abs(a["flux"] - b["flux"]) <= tol[1] * max(abs(b["flux"]), 1e-30), (what, a["flux"], b["flux"])


@pytest.mark.parametrize("arrangement", ["default", "chained-serial"])
@pytest.mark.parametrize("ny", E.STATIC_NY)
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_ib_walls_and_corners(gpu, oracle, precision, ny, arrangement):
    """41 static points on rows 0 and YDIM-1, in the corners (0, 0) and (XDIM-1, YDIM-1), on half-integers
    and coincident (ib_edges.wall_points) on 384 x 131 (the top wall in a three-row ragged chunk) and
    384 x 257 (alone in its chunk), 1 + 6K + 2 iterations in chunks with readers between them.  default: the
    planner's own choice here, the merged chain (its point groups pull the wall rows themselves) with the
    last level beside the deep sweep (odd patch row bound at the top wall); chained-serial: an IB launch
    before every level, the last level behind the deep sweep.  Each against the oracle and both against each
    other; f32 also with full-height level waves, one f64 case also against the one-step path."""
    f64 = precision == "f64"
    run = _static_run(gpu, oracle, precision, ny, arrangement, **ARRANGEMENTS[arrangement])
    other_name = "chained-serial" if arrangement == "default" else "default"
    other = _static_run(gpu, oracle, precision, ny, other_name, **ARRANGEMENTS[other_name])
    tm = run["tm"]
    assert tm["band_cycles"] >= 5 and tm["sweepk_launches"] >= 5, tm
    dflt, chained = (run, other) if arrangement == "default" else (other, run)
    if arrangement == "default":  # the merged chain ran, side by side with the deep sweep
        assert tm["band_par_cycles"] == tm["band_cycles"] == tm["band_merged_cycles"], tm
        # merged: one IB launch per cycle at most (the force owed at its start), chained: K of them
        assert tm["ib_ms"] < 0.6 * chained["tm"]["ib_ms"], (tm, chained["tm"])
    else:
        assert tm["band_par_cycles"] == 0 and tm["band_merged_cycles"] == 0, tm
    _agree(dflt, chained, (1e-13, 1e-11) if f64 else (1e-6, 1e-5), f"static {ny} {precision} default vs chained-serial")
    if not f64 and arrangement == "default":
        full = _static_run(gpu, oracle, precision, ny, "default full-height", IBLB_BAND_VHALF="0")
        assert full["tm"]["band_cycles"] >= 5
        # half-height waves ran: fewer cells where a 256-row chunk is not the whole column anyway
        assert tm["fused_cells"] < full["tm"]["fused_cells"] or (ny <= 256 and tm["fused_cells"] == full["tm"]["fused_cells"]), \
            (tm, full["tm"])
        _agree(run, full, (1e-6, 1e-5), f"static {ny} f32 half-height vs full-height")
    if f64 and arrangement == "default" and ny == E.STATIC_NY[0]:
        one = _static_run(gpu, oracle, precision, ny, "one-step", IBLB_IB_BAND="0")
        assert one["tm"]["band_cycles"] == 0 and one["tm"]["sweepk_launches"] == 0, one["tm"]
        _agree(run, one, (1e-13, 1e-12), f"static {ny} f64 band cycle vs one-step path")


# ---- moving points, removal and return --------------------------------------------------------------
_moving_ref = {}


def _moving_reference(O):
    """The oracle over the three phases, computed once: snapshots after phase A, after the first iteration
    without points, after phase B and after phase C."""
    if not _moving_ref:
        from cuda_iblb_11_amd import workloads as W
        nx, ny = E.NX, E.MOVING_NY
        rho, u = W.perturbed_state(nx, ny, E.STATE_SEED[ny])
        sim = O.Simulation(nx, ny, W.TAU, W.TAU2, rho=rho, u=u, body_force=BODY)
        pts = E.moving_schedule(nx, ny)
        marks = {E.PHASE_A: "A", E.PHASE_A + 1: "B1", E.PHASE_A + E.PHASE_B: "B", E.MOVING_STEPS: "C"}
        for it in range(E.MOVING_STEPS):
            sim.set_lagrangian(*pts(it))
            sim.step(1)
            if it + 1 in marks:
                _moving_ref[marks[it + 1]] = _snapshot(sim)
        n = nx * ny  # without points the oracle's force is the body force alone
        assert np.all(_moving_ref["B1"]["force"][:n] == BODY[0]) and np.all(_moving_ref["B1"]["force"][n:] == BODY[1])
    return _moving_ref


def _schedule(points, t0, n):
    ent = [points(it) for it in range(t0, t0 + n)]
    return tuple(np.stack([e[i] for e in ent]) for i in range(3))


def _moving_run(P, O, precision, merge, **knobs):
    """Phases A, B, C on the GPU under the given knobs, each checked against the oracle; returns the fields
    after phase A."""
    from cuda_iblb_11_amd import workloads as W
    nx, ny = E.NX, E.MOVING_NY
    ref = _moving_reference(O)
    env = ENV[f"moving_{nx}x{ny}"]
    assert env["config"]["fields_after"] == [E.PHASE_A, E.PHASE_A + E.PHASE_B, E.MOVING_STEPS]
    ulp_bound = 2 * env["max_fs_ulps"]
    bound = [2 * max(env["max_fields_at"][:i + 1]) for i in range(3)]  # the drift up to that phase
    tag = f"moving {precision} merge {merge} {knobs}"
    pts = E.moving_points(nx, ny)
    rho, u = W.perturbed_state(nx, ny, E.STATE_SEED[ny])
    with _knobs(IBLB_BAND_MERGE=merge, **knobs):
        lat = P.Lattice(nx, ny, W.TAU, W.TAU2, precision=precision, body_force=BODY, max_points=4096)
        try:
            lat.set_state(rho, u)
            lat.set_profiling(True)
            # phase A: boot, 3 + 2 + 3 band cycles, a new plan whenever a filament reaches new rows
            t = 0
            for n in (1, 3 * K, 2 * K + 1, 3 * K):
                lat.set_lagrangian_steps(*_schedule(pts, t, n))
                lat.step(n)
                t += n
                lat.macro()
                lat.force()
            assert t == E.PHASE_A == lat.steps
            tm = tm_a = lat.timing(reset=True)
            print(json.dumps({"case": tag + " A", **{k: tm[k] for k in ("band_cycles", "band_merged_cycles", "band_par_cycles",
                                                                         "sweepk_launches", "fused_cells")}}), flush=True)
            assert tm["band_cycles"] >= 7 and tm["sweepk_launches"] >= 7, tm
            assert tm["band_merged_cycles"] == (tm["band_cycles"] if merge == "2" else 0), tm
            _against(ref["A"], lat, precision, bound[0], ulp_bound, tag + " A")
            for got, want in zip(lat.lagrangian(), pts(E.PHASE_A - 1)):
                assert np.array_equal(got, want)
            after_a = lat.macro()
            # phase B: the points go; one iteration consumes the force they still owe, after it the force
            # is the body force alone, exactly: a force row that a level left behind shows here
            none = np.zeros(0, np.float32)
            lat.set_lagrangian(none, none)
            lat.step(1)
            force = lat.force()
            left = np.flatnonzero(force != ref["B1"]["force"])
            assert left.size == 0, (tag, "force left behind at (component, row, column)",
                                    [(int(j // (nx * ny)), int(j % (nx * ny) // nx), int(j % nx)) for j in left[:8]])
            lat.timing(reset=True)
            lat.step(3 * K)
            tm = lat.timing(reset=True)
            assert tm["sweepk_launches"] == 3 and tm["band_cycles"] == 0, tm  # no-IB deep sweeps
            _against(ref["B"], lat, precision, bound[1], ulp_bound, tag + " B", fs=False, flux=False)
            # phase C: a filament returns over the columns of two earlier patches, across row 256: a stale
            # flag or a stale row of the merged chain's force buffers from phase A shows here
            lat.set_lagrangian(*E.return_points(nx, ny))
            lat.step(E.PHASE_C)
            tm = lat.timing()
            assert tm["band_cycles"] >= 2 and tm["band_merged_cycles"] == (tm["band_cycles"] if merge == "2" else 0), tm
            _against(ref["C"], lat, precision, bound[2], ulp_bound, tag + " C", flux=False)
        finally:
            lat.close()
    return {"macro": after_a, "tm": tm_a}


@pytest.mark.parametrize("merge", ["0", "2"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_ib_moving_rows_then_removed(gpu, oracle, precision, merge):
    """Five filaments on 384 x 601 that sway and shift 0.75 rows per iteration (ib_edges.moving_points): across
    row 128 (the f32 half-chunk and f64 chunk bound) and row 256 (the f32 flag-chunk bound), up onto row
    YDIM-1 and down onto row 0 (clipped there), one standing still whose epsilon goes to 0 in mid-cycle; points
    given ahead per chunk, chained (merge 0) and merged (2) chains.  A: 1 + 8K + 1 iterations against the oracle;
    B: the points removed, the force then exactly the body force and 3K iterations of no-IB deep sweeps;
    C: a static filament over two of the earlier patches.  f32 with half- and full-height level waves."""
    if precision == "f64":
        _moving_run(gpu, oracle, precision, merge)
        return
    half = _moving_run(gpu, oracle, precision, merge, IBLB_BAND_VHALF="1")
    full = _moving_run(gpu, oracle, precision, merge, IBLB_BAND_VHALF="0")
    assert half["tm"]["fused_cells"] < full["tm"]["fused_cells"], (half["tm"], full["tm"])  # half-height waves ran
    _agree(half, full, (1e-6, 1e-5), f"moving f32 merge {merge} half-height vs full-height")
