"""Point schedules (iblb_set_lagrangian_steps) across iblb_step calls, replacements, state resets and
checkpoint restarts, against the oracle stepped one iteration at a time with the points the header's
contract names for every iteration (tests/point_schedule_cases.py; checked on the CPU, with the power of
the bounds below, by tests/test_point_schedule_cases.py).  A lone slab, 256 x 96, f64 and f32.

After every iblb_step call: the step count, and iblb_get_lagrangian equal to the last iteration's points
array for array.  At every check and at the end: rho, ux, uy (each over its maximum), force, F_s and flux
within the bounds of test_gpu_bulk.py::test_moving_points_band_cycle_matches_oracle (the same kernels and
point sets).  The flux is taken at column 100, where the oracle's cumulative flux is no cancelled remainder
at any compared iteration (point_schedule_cases.FLUX_COLUMN has the reason: at the default column it passes
through zero at iteration 2K + 3, where C and E are compared, and a relative bound there measures the
rounding of the terms 80-fold: f32 5.3e-4, f64 4.7e-11 on an MI355X, against 2e-6 .. 5e-6 and 3e-13 .. 7e-13
at the other iterations).  Every comparison prints its figures (pytest -s).
"""
import json

import numpy as np
import pytest

import point_schedule_cases as C

pytestmark = pytest.mark.gpu

K = C.K
N = C.NX * C.NY
_cases, _refs = {}, {}


def case(name):
    if not _cases:
        _cases.update(C.scenarios())
    return _cases[name]


def reference(O, name):
    """The oracle's snapshots of a scenario, computed once for both precisions and left unchanged."""
    if name not in _refs:
        _refs[name] = C.reference(O, case(name))
    return _refs[name]


def lattice(P, precision):
    from cuda_iblb_11_amd import workloads as W
    lat = P.Lattice(C.NX, C.NY, W.TAU, W.TAU2, precision=precision, body_force=C.BODY, max_points=C.MAX_POINTS,
                    flux_column=C.FLUX_COLUMN)
    lat.set_profiling(True)
    return lat


def against(lat, snap, precision, what):
    """Fields, force, F_s and flux of lat against an oracle snapshot."""
    rho, u = lat.macro()
    out = {"rho": C.rel(rho, snap["rho"]), "ux": C.rel(u[:N], snap["u"][:N]), "uy": C.rel(u[N:], snap["u"][N:]),
           "force": C.rel(lat.force(), snap["force"]),
           "flux": abs(lat.flux - snap["flux"]) / max(abs(snap["flux"]), 1e-30)}
    if lat.ns > 0:
        assert snap["F_s"].size == 2 * lat.ns, what
        out["F_s"] = C.rel(lat.lagrangian_force(), snap["F_s"])
    print(json.dumps({"case": what, "precision": precision, **out}), flush=True)
    assert max(out["rho"], out["ux"], out["uy"]) <= C.FIELD_TOL[precision], (what, out)
    assert out["force"] <= C.FORCE_TOL[precision], (what, out)
    assert out.get("F_s", 0.0) <= C.FS_TOL[precision], (what, out)
    assert out["flux"] <= C.FLUX_TOL[precision], (what, out)


def points_equal(lat, want, what):
    got = lat.lagrangian()
    assert lat.ns == want[0].size // 2, what
    for a, b in zip(got, want):
        assert np.array_equal(a, b), what


def timing_line(lat, what, reset=False):
    tm = lat.timing(reset=reset)
    print(json.dumps({"case": what, **{k: tm[k] for k in ("band_cycles", "band_merged_cycles", "band_par_cycles",
                                                           "sweepk_launches", "fused_launches")}}), flush=True)
    return tm


def run(lat, sc, actions, points_at, refs, precision, tag, *, g=0, t=0, path=None, after=None):
    """The actions on lat, with the checks every scenario shares.  g: iterations of the scenario so far, t:
    the step count the library must report.  after(action, g): the scenario's own checks.  Returns g."""
    for a in actions:
        if a[0] == "schedule":
            lat.set_lagrangian_steps(*a[1:])
        elif a[0] == "points":
            lat.set_lagrangian(*a[1:])
        elif a[0] == "state":
            lat.set_state(*C.state())
            t = 0
            # the reset: the count restarts, the flux restarts, the points stay those in use before it
            assert lat.steps == 0 and lat.flux == 0.0, (tag, lat.steps, lat.flux)
            points_equal(lat, points_at(g - 1), f"{tag} points after the reset")
        elif a[0] == "save":
            lat.save_checkpoint(path)
        elif a[0] == "step":
            lat.step(a[1])
            g, t = g + a[1], t + a[1]
            assert lat.steps == t, (tag, g, lat.steps, t)
            points_equal(lat, points_at(g - 1), f"{tag} points after iteration {g - 1}")
        elif a[0] == "check":
            against(lat, refs[g], precision, f"{tag} {a[1]} (after {g})")
        if after:
            after(a, g)
    against(lat, refs[g], precision, f"{tag} end (after {g})")
    return g


def twin_macro(P, sc):
    """The scenario's iterations as iblb_set_lagrangian + iblb_step(1) each (f64)."""
    lat = lattice(P, "f64")
    try:
        lat.set_state(*C.state())
        for g in range(sc.steps):
            lat.set_lagrangian(*sc.points_at(g))
            lat.step(1)
        return lat.macro()
    finally:
        lat.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_schedule_across_calls(gpu, oracle, name, precision):
    """A: one schedule of 1 + 3K + 5 entries consumed by calls of 1, K, 2, K + 3, K iterations: band cycles
    that start at offsets 1, 1 + K + 2 and 1 + 2K + 5 into it.  B: K + 3 entries and calls of 1, 2K, K + 1:
    the schedule runs out inside the second band cycle and its last entry is held.  f64: also against a
    context fed iblb_set_lagrangian + iblb_step(1) per iteration, within the bounds of
    test_gpu_bulk.py::test_schedule_equals_per_iteration_points."""
    sc = case(name)
    lat = lattice(gpu, precision)
    try:
        lat.set_state(*C.state())
        run(lat, sc, sc.actions, sc.points_at, reference(oracle, name), precision, f"{name} {precision}")
        tm = timing_line(lat, f"{name} {precision}")
        assert tm["band_cycles"] >= 2, tm
        if precision == "f64":
            r1, u1 = lat.macro()
            r0, u0 = twin_macro(gpu, sc)
            d = (C.rel(r1, r0), C.rel(u1, u0))
            print(json.dumps({"case": f"{name} schedule vs per-iteration points", "rho": d[0], "u": d[1]}), flush=True)
            assert d[0] <= 1e-13 and d[1] <= 1e-12, d
    finally:
        lat.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_schedule_replaced_removed_and_static(gpu, oracle, precision):
    """C: a schedule on 3 filaments replaced in mid-schedule by one on 2 (the force owed to the old points
    evaluated first, the point count changing), removed by a schedule of no points (one iteration consumes
    the owed force; after it the force is the body force exactly and K iterations are one no-IB deep launch),
    then static points.  Against the oracle after each phase."""
    sc = case("C")
    lat = lattice(gpu, precision)
    seen = []

    def after(a, g):
        if a == ("check", "points gone"):
            force = lat.force()
            left = np.flatnonzero(np.concatenate([force[:N] != C.BODY[0], force[N:] != C.BODY[1]]))
            assert left.size == 0, ("force left behind at (component, row, column)",
                                    [(int(j // N), int(j % N // C.NX), int(j % C.NX)) for j in left[:8]])
            lat.timing(reset=True)
            seen.append("gone")
        elif a == ("check", "no points"):
            tm = timing_line(lat, f"C {precision} no points", reset=True)
            assert tm["sweepk_launches"] == 1 and tm["band_cycles"] == 0, tm
            seen.append("deep")

    try:
        lat.set_state(*C.state())
        run(lat, sc, sc.actions, sc.points_at, reference(oracle, "C"), precision, f"C {precision}", after=after)
        assert seen == ["gone", "deep"]
        timing_line(lat, f"C {precision} static points")
    finally:
        lat.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_entries_that_differ_in_velocity_and_epsilon_only(gpu, oracle, precision):
    """D: fixed positions (one band plan for every cycle), u_s changing every entry and one point's epsilon
    going to 0 inside the first band cycle."""
    sc = case("D")
    lat = lattice(gpu, precision)
    try:
        lat.set_state(*C.state())
        run(lat, sc, sc.actions, sc.points_at, reference(oracle, "D"), precision, f"D {precision}")
        assert timing_line(lat, f"D {precision}")["band_cycles"] >= 1
    finally:
        lat.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_set_state_rebases_the_schedule(gpu, oracle, precision):
    """E: iblb_set_state K + 2 iterations into a schedule that began at iteration 1 + K (before it a static
    line of 40 points at x = 40.3).  The schedule stays and restarts with the state: the step count
    and the flux restart at 0, iblb_get_lagrangian returns the points in use before the reset until the first
    step, and iteration i of the new state uses entry i: 1 + 2K iterations in one call (boot and two band
    cycles) against a fresh oracle.  Before the re-base the schedule kept its old t0: entry 0 for the first
    1 + K iterations, and the first cycle's bands planned around the points from before the schedule
    (tests/test_point_schedule_cases.py shows that mapping 1.4x max|u| away from this reference)."""
    sc = case("E")
    lat = lattice(gpu, precision)

    def after(a, g):
        if a[0] == "state":
            lat.timing(reset=True)

    try:
        lat.set_state(*C.state())
        run(lat, sc, sc.actions, sc.points_at, reference(oracle, "E"), precision, f"E {precision}", after=after)
        assert lat.steps == 1 + 2 * K
        assert timing_line(lat, f"E {precision} after the reset")["band_cycles"] >= 1
    finally:
        lat.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_checkpoint_under_a_schedule(gpu, oracle, tmp_path, precision):
    """F: a checkpoint K + 3 iterations into a schedule of 1 + 3K entries holds the entry in use.  A fresh
    context restored from it reports the saved step count, point count and points; continued (the remaining
    entries given as a new schedule) it agrees with the uninterrupted run (f64: 1e-13 absolute, the bound of
    test_gpu_fused.py::test_checkpoint_restart with IB; f32: 1e-4 relative) and with the oracle; held
    (stepped K + 1 with nothing set) it agrees with the oracle holding the saved points."""
    sc = case("F")
    refs = reference(oracle, "F")
    ck = str(tmp_path / "schedule.ck")
    lat = lattice(gpu, precision)
    try:
        lat.set_state(*C.state())
        run(lat, sc, sc.actions, sc.points_at, refs, precision, f"F {precision}", path=ck)
        assert timing_line(lat, f"F {precision}")["band_cycles"] >= 1
        r1, u1 = lat.macro()
    finally:
        lat.close()
    save = sc.saved_at
    for rname, acts in sc.restarts.items():
        at = sc.restart_points_at[rname]
        tag = f"F {precision} {rname}"
        b = lattice(gpu, precision)
        try:
            assert acts[0] == ("load",)
            b.load_checkpoint(ck)
            assert b.steps == save, (tag, b.steps)
            points_equal(b, sc.points_at(save - 1), f"{tag} points after the load")
            if rname == "held":
                end = save + sum(a[1] for a in acts if a[0] == "step")
                _, got = C.oracle_run(oracle, at, 0, end, marks=(end,))
                refs_b = got
            else:
                refs_b = refs
            run(b, sc, acts[1:], at, refs_b, precision, tag, g=save, t=save)
            assert timing_line(b, tag)["band_cycles"] >= 1
            if rname == "continued":
                r2, u2 = b.macro()
                if precision == "f64":
                    d = (float(np.max(np.abs(r1 - r2))), float(np.max(np.abs(u1 - u2))))
                    bound = 1e-13
                else:
                    d = (C.rel(r2, r1), C.rel(u2, u1))
                    bound = 1e-4
                print(json.dumps({"case": f"{tag} vs uninterrupted", "rho": d[0], "u": d[1], "bound": bound}), flush=True)
                assert max(d) <= bound, (tag, d)
        finally:
            b.close()


def test_errors_leave_the_schedule_working(gpu, oracle):
    """iblb_set_lagrangian_steps refuses nsteps < 1 and ns > max_points (IBLB_ERR_ARG) and, with the cilia
    kinematics active, any schedule (IBLB_ERR_STATE); after each refused call on an active schedule the
    remaining entries are used as before (B's schedule and calls, f64, against the oracle)."""
    sc = case("B")
    refs = reference(oracle, "B")
    bad = [(np.zeros((0, 2 * C.MAX_POINTS), np.float32),) * 2,          # nsteps = 0
           (np.zeros((2, 2 * (C.MAX_POINTS + 1)), np.float32),) * 2]    # ns = max_points + 1
    lat = lattice(gpu, "f64")
    try:
        lat.set_state(*C.state())
        g = run(lat, sc, sc.actions[:2], sc.points_at, refs, "f64", "errors start")
        for args, step in zip(bad, sc.actions[2:]):
            with pytest.raises(gpu.IblbError) as err:
                lat.set_lagrangian_steps(*args)
            assert err.value.code == gpu.IBLB_ERR_ARG, err.value
            g = run(lat, sc, [step], sc.points_at, refs, "f64", f"errors after a refused call ({g})", g=g, t=g)
        assert g == sc.steps
    finally:
        lat.close()
    cil = lattice(gpu, "f64")
    try:
        cil.set_state()
        cil.set_cilia(1, float(C.NX), 100000, 100000)
        with pytest.raises(gpu.IblbError) as err:
            cil.set_lagrangian_steps(*sc.actions[0][1:])
        assert err.value.code == gpu.IBLB_ERR_STATE, err.value
    finally:
        cil.close()
