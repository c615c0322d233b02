"""The on-device cilia (iblb_set_cilia) on every path iblb_step can take, against the oracle twin of
tests/cilia_cases.py (checked on the CPU by tests/test_cilia_cases.py): oracle.Simulation stepped one
iteration at a time with oracle.Cilia.points(it).

The kinematics keep state across iterations (cil_lasts, cil_bpoints), and a lost hand-over heals in the points
after one iteration while the fields stay wrong by orders of magnitude (test_cilia_cases.py), so every case
compares rho, u_x, u_y with the twin (1e-9 in f64, 1e-4 in f32, each relative to its maximum: the bounds of
tests/test_gpu_fused.py::test_cilia_band_cycle), and after every call the points, u_s and epsilon of
lagrangian() with Cilia.s / u_s / epsilon bit for bit.  The fields are read at the end of a case (and where a
case says so), not after every call: a field read evaluates the force the state owes, and the hand-over with
that force still owed is one of the paths under test.  The band-cycle and deep-launch counts of timing() pin
the path the title names.

What the band planner does with the two configurations is host code (csrc/band_plan.h), settled on the CPU
with tests/band_plan_main.cpp on the points of cilia_cases.cycle_points: a lone WIDE slab (512 x 192) is
accepted at depths 4, 5 and 7 in f64 and f32 (trapezoids over 115712 / 152320 / 234752 cells a cycle, below
half the cycle's lattice updates); a lone REF slab (288 x 192) is declined at every depth (177280 cells
against 138240 at depth 5), so there a call of >= K iterations runs the kinematics ahead into a schedule and
then takes its entries in one-step iterations.  A REF slab of an RCCL group has no such rule and runs band
cycles (tests/mock_rccl/run_cilia.py).

Every test prints its worst figure as a ratio to its bound.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import average_ref as R
import cilia_cases as CC
import tracer_ref as T
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W

pytestmark = pytest.mark.gpu

K = CC.K
PRECISIONS = ["f64", "f32"]
# two contexts of one build that differ in the order of the spread's atomics only: the bounds of
# tests/test_gpu_fused.py::test_local_slab_group (f64) and tests/mock_rccl/run_group.py (f32)
SAME_BUILD = {"f64": 1e-12, "f32": 1e-5}
FS_TOL = {"f64": 1e-5, "f32": 1e-2}  # F_s against the oracle: the bounds of tests/point_schedule_cases.py


@functools.lru_cache(maxsize=None)
def twin(name):
    """The oracle twin's snapshots after every call of a case, computed once for f64 and f32."""
    from oracle import oracle as O
    O.load()
    cfg, actions = {
        "case1 depth4": (CC.WIDE, CC.case1(4)), "case1 depth5": (CC.WIDE, CC.case1(5)[:4]),
        "case2 WIDE": (CC.WIDE, CC.CASE2_WIDE), "case2 REF": (CC.REF, CC.CASE2_REF),
        "case3 cycle": (CC.WIDE, CC.steps(*CC.CASE3["cycle"])), "case3 owed": (CC.WIDE, CC.steps(*CC.CASE3["owed"])),
        "case4": (CC.WIDE, CC.steps(CC.CASE4_STEPS)), "case5": (CC.WIDE, CC.case5()), "case6": (CC.REF, CC.CASE6),
        "group WIDE": (CC.WIDE, CC.steps(*CC.GROUP_CALLS)), "group REF": (CC.REF, CC.steps(*CC.GROUP_CALLS)),
    }[name]
    return CC.run_twin(O, cfg, actions)[1]


def new_lattice(gpu, cfg, precision, cilia=True, state=True, **kw):
    lat = gpu.Lattice(cfg.nx, cfg.ny, W.TAU, W.TAU2, precision=precision, body_force=CC.BODY,
                      max_points=cfg.max_points, **kw)
    if cilia:  # before the state: the kinematics start at the context's iteration with zeroed history
        lat.set_cilia(*cfg.cilia)
    if state:
        lat.set_state(*cfg.state())
    return lat


def check_points(lat, snap, what):
    s, us, eps = lat.lagrangian()
    assert np.array_equal(s, snap["s"]), (what, "s", snap["g"])
    assert np.array_equal(us, snap["u_s"]), (what, "u_s", snap["g"])
    assert np.array_equal(eps, snap["eps"]), (what, "epsilon", snap["g"])


def check_fields(rho, u, snap, precision, what):
    r = CC.fields_rel(rho, u, snap["rho"], snap["u"])
    worst = max(r["rho"], r["ux"], r["uy"])
    print(f"{what} {precision} vs oracle at {snap['g']}: {worst / CC.FIELD_TOL[precision]:.3g} of the bound", r)
    assert worst <= CC.FIELD_TOL[precision], (what, r)


def points_after_every_call(snaps, what):
    return lambda i, lat: check_points(lat, snaps[i], f"{what}, call {i}")


# ---- 1. consecutive schedules, remainders inside ---------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", ["depth4", "depth5"])
def test_consecutive_schedules_with_remainders(gpu, precision, variant, monkeypatch):
    """WIDE.  depth4: calls (1, 2K + 3, K + 1, 2, K) at K = 4, 23 iterations: two cilia schedules back to
    back, each ending in one-step iterations that still take schedule entries, a short call on per-iteration
    kinematics, then a schedule again; >= 4 band cycles.  (At depth 5 that list is 27 iterations, past the
    horizon of 23; cilia_cases.case1.)  depth5: the first four calls of the list at K = 5, 22 iterations,
    >= 3 band cycles.  The planner accepts WIDE at both depths in both precisions.  The same with
    IBLB_IB_BAND=0 (no schedule, no deep launch); f64: both equal each other to 1e-13 (rho) and 1e-11 (u), the
    bounds of test_cilia_band_cycle."""
    depth, actions, cycles = (4, CC.case1(4), 4) if variant == "depth4" else (5, CC.case1(5)[:4], 3)
    monkeypatch.setenv("IBLB_SWEEP_DEPTH", str(depth))
    snaps = twin("case1 " + variant)
    out = {}
    for band in ("1", "0"):
        monkeypatch.setenv("IBLB_IB_BAND", band)
        lat = new_lattice(gpu, CC.WIDE, precision)
        lat.set_profiling(True)
        CC.run_lattice(lat, CC.WIDE, actions, points_after_every_call(snaps, f"case 1 band {band}"))
        assert lat.steps == snaps[-1]["g"]
        rho, u = lat.macro()
        check_fields(rho, u, snaps[-1], precision, f"case 1 {variant} band {band}")
        out[band] = (rho, u, lat.timing())
        lat.close()
    on, off = out["1"][2], out["0"][2]
    assert on["band_cycles"] >= cycles and on["sweepk_launches"] >= cycles, on
    assert off["band_cycles"] == 0 and off["sweepk_launches"] == 0 and off["deep_launches"] == 0, off
    if precision == "f64":
        d = CC.rel(out["1"][0], out["0"][0]), CC.rel(out["1"][1], out["0"][1])
        print(f"case 1 {variant}: band on vs off rho {d[0] / 1e-13:.3g}, u {d[1] / 1e-11:.3g} of the bound")
        assert d[0] <= 1e-13 and d[1] <= 1e-11, d


# ---- 2. iblb_set_state restarts the beat -----------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("config", ["WIDE", "REF"])
def test_set_state_restarts_the_beat(gpu, precision, config, monkeypatch):
    """WIDE at depth 5: step(1 + K + 2), iblb_set_state with another seeded state, step(1 + 2K), step(3):
    schedules and band cycles on both sides of the reset.  REF at the default depth 7: step(4), set_state,
    step(6), step(3), every call shorter than the depth: per-iteration kinematics (no band cycle, no deep
    launch).  The fields are compared after the second and the third call with a twin restarted at the
    reset (fresh Simulation, fresh Cilia, it = 0)."""
    cfg = CC.CONFIGS[config]
    if config == "WIDE":
        monkeypatch.setenv("IBLB_SWEEP_DEPTH", "5")
    else:
        monkeypatch.delenv("IBLB_SWEEP_DEPTH", raising=False)
    actions = CC.CASE2_WIDE if config == "WIDE" else CC.CASE2_REF
    snaps = twin("case2 " + config)
    lat = new_lattice(gpu, cfg, precision)
    cycles = []

    def after(i, lat):
        check_points(lat, snaps[i], f"case 2 {config}, call {i}")
        assert lat.steps == snaps[i]["g"] - (snaps[0]["g"] if i else 0)  # the library's count restarts too
        cycles.append(lat.timing()["band_cycles"])
        if i >= 1:
            rho, u = lat.macro()
            check_fields(rho, u, snaps[i], precision, f"case 2 {config}, call {i}")

    CC.run_lattice(lat, cfg, actions, after)
    tm = lat.timing()
    lat.close()
    if config == "WIDE":
        assert cycles[0] >= 1 and cycles[1] - cycles[0] >= 2, cycles
    else:
        assert tm["band_cycles"] == 0 and tm["deep_launches"] == 0, tm


# ---- 3. checkpoint between band cycles -------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("variant", ["cycle", "owed"])
def test_checkpoint_between_band_cycles(gpu, tmp_path, precision, variant, monkeypatch):
    """WIDE at depth 5.  cycle: step(1 + K), save, step(2K + 2); owed: the save after step(1 + K + 2), whose
    last two iterations are one-step with the force still owed (the load sets it pending).  A fresh context
    with no iblb_set_cilia loads the file and steps 2K + 2.  The restarted run equals the uninterrupted one
    at the IB bounds of test_checkpoint_restart in both precisions (fields 1e-13 absolute, flux 1e-12,
    Lagrangian arrays equal), both equal the oracle, and both ran band cycles after the save."""
    monkeypatch.setenv("IBLB_SWEEP_DEPTH", "5")
    before, rest = CC.CASE3[variant]
    snaps = twin("case3 " + variant)
    a = new_lattice(gpu, CC.WIDE, precision)
    a.step(before)
    check_points(a, snaps[0], "case 3 before the save")
    ck = str(tmp_path / "cilia.ck")
    a.save_checkpoint(ck)
    ca = a.timing()["band_cycles"]
    a.step(rest)
    b = new_lattice(gpu, CC.WIDE, precision, cilia=False, state=False)  # the cilia configuration comes from the file
    b.load_checkpoint(ck)
    assert b.steps == before
    check_points(b, snaps[0], "case 3 after the load")
    b.step(rest)
    assert a.steps == b.steps == before + rest
    for lat, who in ((a, "uninterrupted"), (b, "restarted")):
        check_points(lat, snaps[1], f"case 3 {who}")
    (r1, v1), (r2, v2) = a.macro(), b.macro()
    q1, q2 = a.flux, b.flux
    assert all(np.array_equal(x, y) for x, y in zip(a.lagrangian(), b.lagrangian()))
    cb = b.timing()["band_cycles"]
    ca = a.timing()["band_cycles"] - ca
    a.close()
    b.close()
    check_fields(r1, v1, snaps[1], precision, f"case 3 {variant} uninterrupted")
    check_fields(r2, v2, snaps[1], precision, f"case 3 {variant} restarted")
    d = max(np.max(np.abs(r1 - r2)), np.max(np.abs(v1 - v2)))
    print(f"case 3 {variant} {precision}: restart vs uninterrupted {d / 1e-13:.3g} of the bound, flux "
          f"{abs(q2 - q1) / abs(q1) / 1e-12:.3g}")
    assert d <= 1e-13
    assert abs(q2 - q1) <= 1e-12 * abs(q1), (q1, q2)
    assert ca >= 2 and cb >= 2, (ca, cb)


# ---- 4. observers cut the call ---------------------------------------------------------------------------
AVG = ["rho", "ux", "uy"]


def tracer_seeds(cfg):
    """A 5 x 4 grid away from the walls, seeded offsets of up to half a cell."""
    rng = np.random.default_rng(4)
    x, y = np.meshgrid(np.linspace(60.0, cfg.nx - 62.0, 5), np.linspace(30.0, cfg.ny - 40.0, 4))
    return x.ravel() + rng.uniform(-0.5, 0.5, 20), y.ravel() + rng.uniform(-0.5, 0.5, 20)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("strides", [(6, 4), (6, 12)])
def test_observers_cut_the_call(gpu, precision, strides, monkeypatch):
    """WIDE at depth 5, tracers at stride strides[0] (20 of them) and an average of rho, u_x, u_y with squares
    at stride strides[1], one bin, one step(1 + 20).  (6, 4): the call is cut into pieces 4, 2, 2, 4, ...,
    all shorter than K: per-iteration kinematics, no band cycle.  (6, 12): pieces 6, 6, 6, 3: each piece of 6
    runs the kinematics ahead into a schedule and takes one band cycle.  The twin is a second cilia lattice
    stepped piece by piece, with fields() and host accumulation at every sample and the header's Euler update
    at every tracer event, compared as tests/test_gpu_average.py::test_with_moving_ib_points (sums:
    tol * samples * (1 + max|v|)) and tests/test_gpu_tracers.py::test_trajectory_with_moving_ib_points
    (tol * (path + 1)) compare, tol 1e-9 in f64; in f32 the same-build bound 1e-5.  Final fields: the oracle."""
    monkeypatch.setenv("IBLB_SWEEP_DEPTH", "5")
    ts, av = strides
    cfg, n = CC.WIDE, CC.CASE4_STEPS
    tol = 1e-9 if precision == "f64" else SAME_BUILD["f32"]
    snaps = twin("case4")
    A, B = new_lattice(gpu, cfg, precision), new_lattice(gpu, cfg, precision)
    try:
        x0, y0 = tracer_seeds(cfg)
        A.set_tracers(x0, y0, stride=ts)
        A.set_average(AVG, stride=av, nbins=1, squares=True)
        A.step(n)
        plan = R.pieces([n], 0, tracers=(0, ts), average=(0, av))
        assert sum(p[0] for p in plan) == n
        assert (max(p[0] for p in plan) < K) if strides == (6, 4) else (sum(p[0] >= K for p in plan) == 3)
        x, y, laps, path, samples = x0, y0, np.zeros(20, dtype=np.int32), np.zeros(20), []
        for p, update, sample in plan:
            B.step(p)
            if sample:
                samples.append({k: v.copy() for k, v in B.fields(AVG).items()})
            if update:
                f = B.fields(["ux", "uy"])
                xn, yn, ln = T.advect(f["ux"], f["uy"], x, y, laps, ts)
                path += np.abs(xn - x + (ln - laps) * float(cfg.nx)) + np.abs(yn - y)
                x, y, laps = xn, yn, ln
        assert A.steps == B.steps == n
        check_points(A, snaps[0], "case 4")
        check_points(B, snaps[0], "case 4 twin")
        ref = R.accumulate(samples, 1, squares=True)[0]
        got = A.average(0)
        assert got["samples"] == ref["samples"] == n // av
        worst = 0.0
        for name in AVG:
            vmax = max(np.max(np.abs(s[name])) for s in samples)
            # a sample off by dv <= tol (1 + max|v|) moves its square by 2 |v| dv
            for key, scale in (("sum", 1.0 + vmax), ("sum_sq", 2.0 * vmax * (1.0 + vmax))):
                bound = tol * ref["samples"] * scale
                err = np.max(np.abs(got[key][name] - ref[key][name]))
                worst = max(worst, err / bound)
                assert err <= bound, (name, key, err, bound)
        gx, gy, gl = A.tracers()
        bound = tol * (path + 1.0)
        ex, ey = np.abs(gx - x), np.abs(gy - y)
        print(f"case 4 {strides} {precision}: sums {worst:.3g} of the bound, tracers "
              f"{max(np.max(ex / bound), np.max(ey / bound)):.3g}")
        assert np.array_equal(gl, laps)
        assert np.all(ex <= bound) and np.all(ey <= bound), (ex.max(), ey.max())
        assert A.tracer_info()["updates"] == n // ts and np.max(path) > 0
        rho, u = A.macro()
        check_fields(rho, u, snaps[0], precision, f"case 4 {strides}")
        ta, tb = A.timing(), B.timing()
        if strides == (6, 4):
            assert ta["band_cycles"] == 0 and ta["deep_launches"] == 0, ta
        else:
            assert ta["band_cycles"] >= 1 and ta["band_cycles"] == tb["band_cycles"] == 3, (ta, tb)
    finally:
        A.close()
        B.close()


# ---- 5. cilia off, static points on ----------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_cilia_off_static_points_on(gpu, precision, monkeypatch):
    """WIDE at depth 5: step(1 + K), iblb_set_cilia off, iblb_set_lagrangian with 24 static points,
    step(K + 2); the twin switches its point source at the same iteration.  Before the switch lagrangian()
    returns the last cilia entry and iblb_set_lagrangian is refused with IBLB_ERR_STATE."""
    monkeypatch.setenv("IBLB_SWEEP_DEPTH", "5")
    cfg, actions = CC.WIDE, CC.case5()
    snaps = twin("case5")
    pts = actions[1][1]
    lat = new_lattice(gpu, cfg, precision)
    lat.step(actions[0][1])
    check_points(lat, snaps[0], "case 5 before the switch")
    with pytest.raises(L.IblbError) as e:
        lat.set_lagrangian(*pts)
    assert e.value.code == L.IBLB_ERR_STATE
    check_points(lat, snaps[0], "case 5 after the refusal")
    c0 = lat.timing()["band_cycles"]
    CC.run_lattice(lat, cfg, actions[1:], points_after_every_call(snaps[1:], "case 5"))
    assert lat.steps == snaps[1]["g"]
    rho, u = lat.macro()
    fs = lat.lagrangian_force()
    tm = lat.timing()
    lat.close()
    check_fields(rho, u, snaps[1], precision, "case 5")
    d = CC.rel(fs, snaps[1]["F_s"])
    print(f"case 5 {precision}: F_s {d / FS_TOL[precision]:.3g} of the bound")
    assert d <= FS_TOL[precision]
    assert c0 >= 1 and tm["band_cycles"] - c0 >= 1, (c0, tm)  # the cilia's cycle, then the static points'


@pytest.mark.parametrize("precision", PRECISIONS)
def test_static_points_replaced_elsewhere(gpu, oracle, precision, monkeypatch):
    """What case 5 found, without cilia: static points replaced by static points elsewhere between two calls
    of >= K iterations.  The force the old points owe to the next iteration lies outside the new points' band
    plan, where the cycle's deep sweep applies no IB force; before the fix (a one-step iteration first,
    band_hold_t) it was dropped and then applied K iterations late.  WIDE's lattice at depth 5, step(1 + K),
    new points, step(K + 2), against the oracle.  Measured before the fix: u_x off by 0.35 of its maximum in
    f64 and f32 alike (case 5: 1.07); after it 1.4e-13 / 2.2e-7."""
    monkeypatch.setenv("IBLB_SWEEP_DEPTH", "5")
    cfg = CC.WIDE
    old = W.filament(2, n_points=30, x0=100.3, y0=5.0, dy=1.0, U0=2e-3, period=12, sway=1.0)
    new = CC.static_points(cfg)
    sim = oracle.Simulation(cfg.nx, cfg.ny, W.TAU, W.TAU2, *cfg.state(), body_force=CC.BODY)
    lat = new_lattice(gpu, cfg, precision, cilia=False)
    for pts, n in ((old, 1 + K), (new, K + 2)):
        sim.set_lagrangian(*pts)
        sim.step(n)
        lat.set_lagrangian(*pts)
        lat.step(n)
    rho, u = lat.macro()
    tm = lat.timing()
    lat.close()
    check_fields(rho, u, {"rho": sim.rho, "u": sim.u, "g": 2 * K + 3}, precision, "static points replaced")
    assert tm["band_cycles"] >= 2, tm  # one cycle under each point set


# ---- 6. REF past the existing horizon of paths -----------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("depth", ["5", None])
def test_ref_schedule_without_band_cycles(gpu, precision, depth, monkeypatch):
    """REF, calls (1, 5, 7), 13 iterations, at depth 5 and at the default depth 7.  Neither runs band cycles:
    the planner declines the lone 288 x 192 slab at every depth (module docstring).  At depth 5 both calls,
    at depth 7 the last, run the kinematics ahead into a schedule whose entries one-step iterations take;
    the call of 5 at depth 7 is on per-iteration kinematics."""
    if depth:
        monkeypatch.setenv("IBLB_SWEEP_DEPTH", depth)
    else:
        monkeypatch.delenv("IBLB_SWEEP_DEPTH", raising=False)
    snaps = twin("case6")
    lat = new_lattice(gpu, CC.REF, precision)
    CC.run_lattice(lat, CC.REF, CC.CASE6, points_after_every_call(snaps, "case 6"))
    rho, u = lat.macro()
    tm = lat.timing()
    lat.close()
    check_fields(rho, u, snaps[-1], precision, f"case 6 depth {depth or 7}")
    assert tm["band_cycles"] == 0 and tm["deep_launches"] == 0, tm


# ---- local groups ----------------------------------------------------------------------------------------
_lone = {}


def lone_slab(gpu, cfg, precision):
    """The lone slab through the group's calls, once per configuration and precision."""
    key = (cfg.name, precision)
    if key not in _lone:
        lat = new_lattice(gpu, cfg, precision)
        for n in CC.GROUP_CALLS:
            lat.step(n)
        _lone[key] = lat.macro() + (lat.lagrangian_force(),)
        lat.close()
    return _lone[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("config,nslab", [("REF", 2), ("REF", 3), ("WIDE", 3)])
def test_local_group_cilia(gpu, precision, config, nslab, monkeypatch):
    """iblb_set_cilia on every slab of a local group, iblb_group_step in calls (1, 5, 6): run_cilia inside the
    group step.  REF on 2 slabs: the periodic seam and a cilium base (x = 144) on slab edges; REF on 3; WIDE
    on 3: edges at 170 and 341, inside a cilium's reach.  Gathered fields against the lone slab (1e-13 / 1e-12
    in f64 as test_local_slab_group, 1e-5 in f32 as run_group.py) and the oracle; summed F_s against the lone
    slab's (1e-5); every slab's lagrangian() after every call."""
    monkeypatch.delenv("IBLB_SWEEP_DEPTH", raising=False)
    cfg = CC.CONFIGS[config]
    snaps = twin("group " + config)
    r1, u1, f1 = lone_slab(gpu, cfg, precision)
    rho0, u0 = cfg.state()
    slabs = []
    for xb, xc in gpu.plan_slabs(cfg.nx, nslab):
        s = new_lattice(gpu, cfg, precision, state=False, x_begin=xb, x_count=xc)
        s.set_state(gpu.split_state(rho0, 1, cfg.nx, cfg.ny, xb, xc), gpu.split_state(u0, 2, cfg.nx, cfg.ny, xb, xc))
        slabs.append(s)
    group = gpu.LocalGroup(slabs)
    for i, n in enumerate(CC.GROUP_CALLS):
        group.step(n)
        for s in slabs:
            check_points(s, snaps[i], f"group {config} x {nslab}, slab at {s.x_begin}, call {i}")
    rg, ug = group.gather_macro()
    fs = sum(s.lagrangian_force() for s in slabs)
    for s in slabs:
        s.close()
    check_fields(rg, ug, snaps[-1], precision, f"group {config} x {nslab}")
    tr, tu = (1e-13, 1e-12) if precision == "f64" else (1e-5, 1e-5)
    d = CC.rel(rg, r1), CC.rel(ug, u1), CC.rel(fs, f1)
    print(f"group {config} x {nslab} {precision} vs the lone slab: rho {d[0] / tr:.3g}, u {d[1] / tu:.3g}, "
          f"F_s {d[2] / 1e-5:.3g} of the bound")
    assert d[0] <= tr and d[1] <= tu, d
    assert d[2] <= 1e-5, d


# ---- RCCL slabs ------------------------------------------------------------------------------------------
RCCL_ROWS = [
    # ranks, config, precision, calls, save after call, IBLB_OVERLAP, band cycles expected on every rank
    (2, "WIDE", "f64", "1,12,3,5", 2, "1", 2),
    (4, "WIDE", "f32", "1,12,3,5", None, "1", 2),
    (3, "WIDE", "f64", "1,12,3,5", 2, "1", 2),
    (2, "REF", "f64", "1,5,7", None, "1", 2),
    (3, "REF", "f32", "1,5,7", None, "1", 2),
    (2, "WIDE", "f64", "1,2,3,2,4", None, "1", 0),
    (2, "WIDE", "f64", "1,2,3,2,4", None, "0", 0),
]


@pytest.mark.parametrize("n,config,precision,calls,save,overlap,cycles", RCCL_ROWS)
def test_rccl_slab_cilia(gpu, n, config, precision, calls, save, overlap, cycles):
    """tests/mock_rccl/run_cilia.py at depth 5: every rank attaches, sets the cilia, sets its part of the state
    and steps the calls; the assembled fields against the lone slab and the oracle, lagrangian() per rank bit
    for bit, F_s, gather_macro, and (where `save`) a restart from a checkpoint after that call.

    WIDE 1,12,3,5 on 2 (slabs of 256), 3 (170 / 171: edges inside a cilium's reach) and 4 ranks (128):
    the call of 12 runs two band cycles and two remainders, the call of 5 one; the save after call 2 lies
    between them.  REF 1,5,7 on 2 (seam and a cilium base on the slab edges) and 3 ranks: one cycle per call
    (a group slab has no too-big rule), two in all.  Slabs of 96 and more are >= max(4K, 3K) at K = 5, so
    band_slab_ok holds on every row with IBLB_OVERLAP=1.  WIDE 1,2,3,2,4: every call < K, per-iteration
    kinematics, with the overlapped exchange and (IBLB_OVERLAP=0) without: no band cycle on any rank."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, IBLB_OVERLAP=overlap, IBLB_SWEEP_DEPTH="5", GPU_MAX_HW_QUEUES="16")
    cmd = [sys.executable, os.path.join(here, "mock_rccl", "run_cilia.py"), str(n), config, precision, calls]
    if save is not None:
        cmd.append(str(save))
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, p.stdout + p.stderr[-3000:]
    res = json.loads(lines[-1])
    print(json.dumps(res))
    assert p.returncode == 0 and res["ok"], (res, p.stderr[-2000:])
    assert len(res["band_cycles"]) == n
    if cycles:
        assert all(c >= cycles for c in res["band_cycles"]), res["band_cycles"]
    else:
        assert not any(res["band_cycles"]) and not any(res["deep_launches"]), res
    assert (res["d_restart"] is not None) == (save is not None)
