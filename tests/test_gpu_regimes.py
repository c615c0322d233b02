"""Every collide path against the oracle across the relaxation, Mach and forcing regimes of
tests/regimes.py: the reference-shaped kernels, the one-step kernel with the boot step, the deep
sweeps of the default schedule, the IB one-step path, the IB band cycle and the local slab group.
Every other GPU parity test runs at reference_taus(), amplitude 1e-3 and a body force ~1e-6; each path
receives its collide constants (KConst / Coef) separately, and the f32 assertion there (rho normalised
by ~1, 1e-4) passes a collide that is wrong in one nonlinear or forcing term
(tests/test_regimes.py::test_regimes_discriminate).

Bounds: tests/regimes.py.  Every test prints its figures (one line starting with REGIME) before it
asserts.

Measured on an MI355X.  f32 without IB, worst field / emulation floor: one-step 0.85 ... 1.154 over the
28 cases, deep sweeps <= 1.165 (the figures per pair and FACTOR: tests/regimes.py).  f64: one-step
<= 4.0e-11 (rho - 1; populations 3.5e-11), deep <= 1.8e-12, boot step <= 1.5e-14, with IB <= 1.4e-12 with
force and F_s equal to the oracle's and the band cycle equal to the one-step path.  f32 with IB, per case
(rho - 1, u_x, u_y | force, F_s, flux), against bounds of 1e-4 | 1e-3, 1e-2, 1e-4:
  one-step path, 64 x 192, 30 iterations        band cycle, 256 x 128, 3K + 2 iterations
  Re100    4.9e-7 8.2e-7 7.1e-7 | 3.1e-7 2.3e-7 1.1e-7    5.2e-7 6.3e-7 5.8e-7 | 2.6e-7 2.3e-7 2.6e-7
  swapped  1.1e-6 1.5e-6 1.4e-6 | 5.7e-7 4.7e-7 6.5e-7    9.4e-7 1.1e-6 1.1e-6 | 4.6e-7 3.3e-7 7.7e-7
  BGK      1.7e-6 1.2e-6 1.4e-6 | 7.2e-7 4.7e-7 1.6e-6    1.0e-6 1.0e-6 1.3e-6 | 4.5e-7 3.2e-7 1.3e-6
  Re10     5.9e-7 6.7e-7 6.4e-7 | 6.9e-7 5.2e-7 4.5e-7    7.4e-7 6.8e-7 7.1e-7 | 9.9e-7 9.0e-7 3.8e-7
  Re1      4.3e-7 5.9e-7 3.8e-7 | 2.6e-7 2.6e-7 4.6e-7    5.5e-7 3.1e-7 4.9e-7 | 4.8e-7 3.2e-7 3.8e-7
  magic    9.8e-7 1.0e-6 1.6e-6 | 5.7e-7 4.1e-7 2.7e-7    5.8e-7 1.1e-6 1.4e-6 | 8.6e-7 7.4e-7 1.6e-7
  TODAY    3.2e-7 2.2e-7 2.7e-7 | 1.9e-7 2.1e-7 6.9e-7    4.1e-7 2.6e-7 2.7e-7 | 2.8e-7 2.1e-7 6.1e-7
Every f32 IB path is also held to f32_ib_bound = FACTOR_IB x the floor of the IB emulation, per quantity
(tests/regimes.py; rho - 1, u_x, u_y, force and F_s at 0.80 ... 1.5 x their floors, per path at FACTOR_IB).
The chained and the merged band cycle and the same call on the one-step path give the same rho, u and dense
force bit for bit in all 7 cases (allowed: twice the order envelope, itself 1.3e-7 ... 3.7e-7), and three f32 slabs
the lone lattice's dense force and F_s bit for bit.

The power of the f32 IB assertions on the kernels themselves, by three temporary edits of the library,
each run through the 21 f32 IB tests here (7 one-step, 7 band cycle, 7 slab group) and reverted:
  node_term's rho taken as 1                       21 of 21 fail; the worst quantity >= 132 x its new bound
  a forced cell's make_kforce without the body force 21 of 21 fail; >= 145 x
  macro_out_kernel without the dense force's half    21 of 21 fail (u_x, u_y); >= 6.7e4 x
The earlier bounds also see each of them in every run, but through the fields' 1e-4 only where the error is
small: the first edit at TODAY is 1.78 x that bound (rho - 1 1.78e-4), its dense force is above 1e-3 in 15
of the 21 runs and its F_s above 1e-2 in 1; the second edit's force in 18 and F_s in 11 (smallest margin
2.3 x, BGK with the small body force).  The new bound sees the first two in all five quantities of all runs.
"""
import os

import numpy as np
import pytest

import regimes as R

pytestmark = pytest.mark.gpu

TIGHT, TOL32 = R.TIGHT, R.TOL32
K = int(os.environ.get("IBLB_SWEEP_DEPTH", "7"))  # the library's deep-sweep depth, as tests/test_gpu_fused.py reads it
WD = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
PRECISIONS = ["f64", "f32"]
# bounds with IB: the band tests' (test_gpu_fused.py::test_ib_band_cycle_matches_oracle): f64 fields 1e-10,
# force 1e-9, F_s 1e-5, flux 1e-9; f32 1e-4, 1e-3, 1e-2, 1e-4, and in f32 the floor's bound besides (_check_ib)
IB_TOL = R.IB_TOL


def _report(test, c, precision, **figures):
    print("REGIME", test, c if isinstance(c, str) else c.id, precision,
          " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


def _lattice(P, c, nx, ny, precision, **kw):
    return P.Lattice(nx, ny, c.tau, c.tau2, precision=precision, body_force=c.force, **kw)


def _check_no_ib(test, O, lat, c, nx, ny, steps, precision, flux):
    """Fields, populations and flux of a no-IB run against the oracle; returns the populations."""
    sim = R.oracle_run(O, c, nx, ny, steps, flux_column=flux["flux_column"], flux_norm=flux["flux_norm"])
    rho, u = lat.macro()
    e = R.field_errors(rho, u, sim.rho, sim.u)
    f = lat.populations()
    w = np.tile(WD, nx * ny)
    e_f = float(np.max(np.abs(f - sim.f)) / np.max(np.abs(sim.f - w)))
    d_q = abs(lat.flux - sim.flux)
    if precision == "f64":
        _report(test, c, precision, nx=nx, ny=ny, **e, f=e_f, flux=d_q / abs(sim.flux))
        assert max(e.values()) <= TIGHT, e
        assert R.rel(f, sim.f) <= TIGHT and e_f <= TIGHT
        assert d_q <= TIGHT * abs(sim.flux), (lat.flux, sim.flux)
    else:
        fl = R.floor(O, c, nx, ny, steps)
        _report(test, c, precision, nx=nx, ny=ny, **e, f=e_f, flux=d_q / sim.flux_scale, floor=fl,
                ratio=max(e.values()) / fl, f_ratio=e_f / fl)
        bound = R.f32_bound(O, c, nx, ny, steps)
        assert max(e.values()) <= bound, (e, bound)
        assert e_f <= 3 * bound, (e_f, bound)
        # the flux sums YDIM u_x / flux_norm per iteration, each within the u_x bound of max|u_x|
        assert d_q <= 3 * bound * sim.flux_scale, (lat.flux, sim.flux, sim.flux_scale)
    assert lat.count_nonfinite() == 0
    assert lat.steps == steps
    return f


# ---- a. the reference-shaped kernels ---------------------------------------------------------------
@pytest.mark.parametrize("pair", list(R.TAUS))
def test_equilibrium_collision_bitexact_regimes(gpu, oracle, pair):
    """iblb_equilibrium + iblb_collision equal the oracle's bit for bit (the assertion of
    test_gpu_kernels.py::test_equilibrium_collision_bitexact) at every relaxation pair, on a state of
    amplitude 3e-2 with a per-cell force of 1e-3 U(-1, 1) and populations w (1 + 3e-2 U)."""
    import torch
    from cuda_iblb_11_amd import kernels as KR
    tau, tau2 = R.TAUS[pair]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    for X, Y in [(72, 40), (5, 3)]:
        rng = np.random.default_rng(1)
        n = X * Y
        rho = 1.0 + 3e-2 * rng.uniform(-1, 1, n)
        u = 3e-2 * rng.uniform(-1, 1, 2 * n)
        force = 1e-3 * rng.uniform(-1, 1, 2 * n)
        f = np.tile(WD, n) * (1 + 3e-2 * rng.uniform(-1, 1, 9 * n))
        f0o, Fo, f1o = np.zeros(9 * n), np.zeros(9 * n), np.zeros(9 * n)
        oracle.equilibrium(u, rho, f0o, force, Fo, X, Y, tau)
        oracle.collision(f0o, f, f1o, Fo, tau, tau2, X, Y, 0)
        df0 = torch.zeros(9 * n, dtype=torch.float64, device="cuda")
        dF, df1 = torch.zeros_like(df0), torch.zeros_like(df0)
        KR.equilibrium(dev(u), dev(rho), df0, dev(force), dF, X, Y, tau)
        KR.collision(df0, dev(f), df1, dF, tau, tau2, X, Y, 0)
        torch.cuda.synchronize()
        assert np.array_equal(df0.cpu().numpy(), f0o), (pair, X, Y)
        assert np.array_equal(dF.cpu().numpy(), Fo), (pair, X, Y)
        assert np.array_equal(df1.cpu().numpy(), f1o), (pair, X, Y)


# ---- b. the one-step kernel and the boot step --------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", R.FULL, ids=R.ids(R.FULL))
def test_one_step_matches_oracle(gpu, oracle, c, precision, monkeypatch):
    """IBLB_SWEEP=0: the boot step and 59 one-step launches, 48 x 40, with a flux column and a flux norm
    that are not the defaults; rho - 1, u_x, u_y, the populations and the flux against the oracle."""
    monkeypatch.setenv("IBLB_SWEEP", "0")
    (nx, ny), steps = R.SHAPE, R.STEPS
    flux = {"flux_column": nx // 3, "flux_norm": float(ny)}
    lat = _lattice(gpu, c, nx, ny, precision, **flux)
    try:
        lat.set_state(*R.state(c, nx, ny))
        lat.step(steps)
        _check_no_ib("one_step", oracle, lat, c, nx, ny, steps, precision, flux)
    finally:
        lat.close()


@pytest.mark.parametrize("pair", list(R.TAUS))
def test_boot_step_regimes(gpu, oracle, pair):
    """One step from set_state (the boot collide, given rho and u explicitly) at every relaxation pair,
    amplitude 3e-2, body force (1e-4, -5e-5): one reference iteration within 1e-12 (f64 rounding of a
    few operations on values ~1, relative to fields ~1e-2; test_gpu_fused.py::test_boot_step_and_initial_state)."""
    c = R.case(pair, 3e-2, "big")
    nx, ny = 40, 30
    rho, u = R.state(c, nx, ny, 3)
    lat = _lattice(gpu, c, nx, ny, "f64")
    try:
        lat.set_state(rho, u)
        r0, u0 = lat.macro()
        assert np.array_equal(r0, rho) and np.array_equal(u0, u)
        sim = oracle.Simulation(nx, ny, c.tau, c.tau2, rho=rho, u=u, body_force=c.force)
        sim.step(1)
        lat.step(1)
        e = R.field_errors(*lat.macro(), sim.rho, sim.u)
        e_f = R.rel(lat.populations(), sim.f)
        _report("boot", c, "f64", **e, f=e_f)
        assert max(e.values()) <= 1e-12 and e_f <= 1e-12, (e, e_f)
    finally:
        lat.close()


# ---- c. the default schedule: deep sweeps -------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", R.CORNERS, ids=R.ids(R.CORNERS))
def test_default_schedule_regimes(gpu, oracle, c, precision, monkeypatch):
    """No IBLB_* knob set (but the depth the suite runs at): one call of 1 + 2K + 2 iterations = boot, two
    deep sweeps, a remainder, on ragged shapes; against the oracle, and the populations bit-identical to
    the same call under IBLB_SWEEP=0 (the contract of test_sweep_deep_bit_identical)."""
    for name in [n for n in os.environ if n.startswith("IBLB_") and n != "IBLB_SWEEP_DEPTH"]:
        monkeypatch.delenv(name)
    steps = 1 + 2 * K + 2
    for nx, ny in [(70, 125), (3, 130)]:
        flux = {"flux_column": nx // 3, "flux_norm": float(ny)}
        out = {}
        for sweep in (None, "0"):
            if sweep is not None:
                monkeypatch.setenv("IBLB_SWEEP", sweep)
            lat = _lattice(gpu, c, nx, ny, precision, **flux)
            try:
                lat.set_state(*R.state(c, nx, ny))
                lat.step(steps)
                tm = lat.timing()
                if sweep is None:
                    assert tm["deep_launches"] >= 2, tm
                    f = _check_no_ib("deep", oracle, lat, c, nx, ny, steps, precision, flux)
                else:
                    assert tm["deep_launches"] == 0, tm
                    f = lat.populations()
                out[sweep] = (f, lat.flux)
            finally:
                lat.close()
        monkeypatch.delenv("IBLB_SWEEP")
        assert np.array_equal(out[None][0], out["0"][0]), (nx, ny, float(np.max(np.abs(out[None][0] - out["0"][0]))))
        assert abs(out[None][1] - out["0"][1]) <= 1e-12 * abs(out["0"][1]), (out[None][1], out["0"][1])


# ---- d, e. the IB paths -------------------------------------------------------------------------------
def _check_ib(test, O, lat, sim, c, precision, cfg=None, **extra):
    """Fields, dense force, F_s and flux of an IB run against the oracle at the suite's bounds (IB_TOL); in
    f32 also at the floor's bound of the configuration cfg = (nx, ny, steps, points): every quantity within
    f32_ib_bound (FACTOR_IB x the emulation's floor), the flux as _check_no_ib bounds it."""
    e = R.field_errors(*lat.macro(), sim.rho, sim.u)
    e_force = R.rel(lat.force(), sim.force)
    e_fs = R.rel(lat.lagrangian_force(), sim.F_s)
    d_q = abs(lat.flux - sim.flux)
    e_q = d_q / max(abs(sim.flux), 1e-30)
    if precision == "f32":
        fl = R.ib_floor(O, c, *cfg)
        got = {**e, "force": e_force, "F_s": e_fs}
        extra = dict(extra, **{"floor_" + q: fl[q] for q in fl}, **{"ratio_" + q: got[q] / fl[q] for q in fl},
                     ratio=max(got[q] / fl[q] for q in fl), flux_abs=d_q / sim.flux_scale)
    _report(test, c, precision, **e, force=e_force, F_s=e_fs, flux=e_q, **extra)
    tol = IB_TOL[precision]
    assert max(e.values()) <= tol["fields"], e
    assert e_force <= tol["force"] and e_fs <= tol["F_s"] and e_q <= tol["flux"], (e_force, e_fs, e_q)
    if precision == "f32":
        bound = R.f32_ib_bound(O, c, *cfg)
        for q in fl:
            assert got[q] <= bound[q], (q, got[q], bound[q], fl[q])
        # the flux sums YDIM u_x / flux_norm per iteration, each within the u_x bound of max|u_x|
        assert d_q <= 3 * bound["ux"] * sim.flux_scale, (lat.flux, sim.flux, sim.flux_scale)
    assert lat.count_nonfinite() == 0


def _within_envelope(test, c, a, b, env, factor, quantities):
    """Readers a against b (rho, u, force, F_s) within factor x the order envelope, per quantity; bit for
    bit where the envelope is 0."""
    d = R.ib_errors(*a, *b)
    _report(test, c, "f32", **{q: d[q] for q in quantities}, **{"env_" + q: env[q] for q in quantities})
    for q in quantities:
        assert d[q] <= factor * env[q] if env[q] > 0 else d[q] == 0, (q, d[q], env[q])


def _readers(lat):
    return (*lat.macro(), lat.force(), lat.lagrangian_force())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", R.IB_CASES, ids=R.ids(R.IB_CASES))
def test_ib_one_step_regimes(gpu, oracle, c, precision):
    """The IB one-step path (ib_point_kernel), 64 x 192 over 30 iterations, points given every iteration: the
    moving points of test_ib_edges_and_epsilon (at x ~ 0 and x ~ XDIM, masked ones) at the case's IB speed.
    f32: every quantity within FACTOR_IB x the floor of the IB emulation."""
    nx, ny, steps, _ = R.IB_CONFIGS["edge"]
    pts = R.edge_points(nx, c.ib_amp)
    rho, u = R.state(c, nx, ny)
    sim = R.ib_oracle_run(oracle, c, nx, ny, steps, "edge")
    lat = _lattice(gpu, c, nx, ny, precision, max_points=4096)
    try:
        lat.set_state(rho, u)
        for it in range(steps):
            lat.set_lagrangian(*pts(it))
            lat.step(1)
        _check_ib("ib_one_step", oracle, lat, sim, c, precision, (nx, ny, steps, "edge"))
    finally:
        lat.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", R.IB_CASES, ids=R.ids(R.IB_CASES))
def test_ib_band_cycle_regimes(gpu, oracle, c, precision, monkeypatch):
    """The IB band cycle, 256 x 128 with a standing 40-point line at the case's IB speed: one call of
    3K + 2 iterations under IBLB_IB_BAND=1 against the oracle, and in f64 against the same call on the
    one-step path (IBLB_IB_BAND=0) within 1e-10 (equal up to the arrival order of the spread atomics).
    f32: the band cycle as the library picks it, chained (IBLB_BAND_MERGE=0: ib_ghost_kernel and the levels)
    and merged (IBLB_BAND_MERGE=2: ib_next_group), each within FACTOR_IB x the floor of the IB emulation; and
    the same call on the one-step path against each of them on rho - 1, u and the dense force within twice
    the order envelope (bit for bit where the envelope is 0)."""
    nx, ny, steps = 256, 128, 3 * K + 2
    cfg = (nx, ny, steps, "line")
    pts = R.line(100.0, 40, amp=c.ib_amp)
    rho, u = R.state(c, nx, ny, R.IB_CONFIGS["line"][3])
    sim = R.ib_oracle_run(oracle, c, *cfg)
    out = {}
    runs = [("1", None), ("0", None)] if precision == "f64" else [("1", None), ("1", "0"), ("1", "2"), ("0", None)]
    for band, merge in runs:
        monkeypatch.setenv("IBLB_IB_BAND", band)
        if merge is None:
            monkeypatch.delenv("IBLB_BAND_MERGE", raising=False)
        else:
            monkeypatch.setenv("IBLB_BAND_MERGE", merge)
        lat = _lattice(gpu, c, nx, ny, precision, max_points=4096)
        try:
            lat.set_state(rho, u)
            lat.set_lagrangian(*pts)
            lat.set_profiling(True)
            lat.step(steps)
            n_deep = lat.timing()["sweepk_launches"]
            assert n_deep >= 3 if band == "1" else n_deep == 0, lat.timing()
            name = "ib_band" + band + ("" if merge is None else "_merge" + merge)
            _check_ib(name, oracle, lat, sim, c, precision, cfg, sweepk_launches=n_deep)
            out[band, merge] = _readers(lat)
        finally:
            lat.close()
    if precision == "f64":
        d = [R.rel(a, b) for a, b in zip(out["1", None][:3], out["0", None][:3])]
        _report("ib_band_vs_one_step", c, precision, rho=d[0], u=d[1], force=d[2])
        assert max(d) <= 1e-10, d
    else:
        env = R.ib_order_envelope(c, *cfg)
        for merge in (None, "0", "2"):
            _within_envelope("ib_band_vs_one_step_merge" + str(merge), c, out["1", merge], out["0", None], env, 2,
                             ("rho-1", "ux", "uy", "force"))


@pytest.mark.parametrize("c", R.IB_CASES, ids=R.ids(R.IB_CASES))
def test_ib_local_slab_group_regimes(gpu, oracle, c):
    """Three f32 x-slabs of the 64 x 192 lattice with edge_points given every iteration over 30 iterations
    (ib_ghost_kernel: the points at x ~ 0 and x ~ XDIM reach slabs 0 and 2 as images across the lattice's
    seam): every quantity against the oracle within FACTOR_IB x the floor of the IB emulation, and the dense
    force and F_s against the lone f32 lattice's within the order envelope."""
    nx, ny, steps, _ = R.IB_CONFIGS["edge"]
    cfg = (nx, ny, steps, "edge")
    pts = R.edge_points(nx, c.ib_amp)
    rho, u = R.state(c, nx, ny)
    sim = R.ib_oracle_run(oracle, c, *cfg)
    single = _lattice(gpu, c, nx, ny, "f32", max_points=4096)
    slabs = []
    try:
        single.set_state(rho, u)
        for xb, xc in gpu.plan_slabs(nx, 3):
            s = _lattice(gpu, c, nx, ny, "f32", x_begin=xb, x_count=xc, max_points=4096)
            slabs.append(s)
            s.set_state(gpu.split_state(rho, 1, nx, ny, xb, xc), gpu.split_state(u, 2, nx, ny, xb, xc))
        group = gpu.LocalGroup(slabs)
        for it in range(steps):
            for s in slabs + [single]:
                s.set_lagrangian(*pts(it))
            single.step(1)
            group.step(1)

        class Gathered:  # the group's readers in the lone lattice's layout
            macro = staticmethod(group.gather_macro)
            flux = group.flux

            @staticmethod
            def force():
                f = np.empty((2, ny, nx))
                for s in slabs:
                    f[:, :, s.x_begin:s.x_begin + s.x_count] = s.force().reshape(2, ny, s.x_count)
                return f.ravel()

            @staticmethod
            def lagrangian_force():  # each point's F_s is reported by one slab (zeros elsewhere)
                return sum(s.lagrangian_force() for s in slabs)

            @staticmethod
            def count_nonfinite():
                return sum(s.count_nonfinite() for s in slabs)

        _check_ib("ib_slab_group", oracle, Gathered, sim, c, "f32", cfg)
        env = R.ib_order_envelope(c, *cfg)
        _within_envelope("ib_slab_group_vs_lone", c, _readers(Gathered), _readers(single), env, 1, ("force", "F_s"))
    finally:
        for s in slabs + [single]:
            s.close()


# ---- f. the local slab group ----------------------------------------------------------------------------
@pytest.mark.parametrize("nslab", [2, 3])
@pytest.mark.parametrize("c", R.CORNERS[:2], ids=R.ids(R.CORNERS[:2]))
def test_local_slab_group_regimes(gpu, c, nslab):
    """2 and 3 x-slabs of a 48 x 40 lattice (the slab-edge kernels, local transport) over 20 iterations
    without IB: bit-identical to the single slab (the contract of test_local_slab_group)."""
    (nx, ny), steps = R.SHAPE, 20
    rho, u = R.state(c, nx, ny, 9)
    single = _lattice(gpu, c, nx, ny, "f64")
    slabs = []
    try:
        single.set_state(rho, u)
        for xb, xc in gpu.plan_slabs(nx, nslab):
            s = _lattice(gpu, c, nx, ny, "f64", x_begin=xb, x_count=xc)
            slabs.append(s)
            s.set_state(gpu.split_state(rho, 1, nx, ny, xb, xc), gpu.split_state(u, 2, nx, ny, xb, xc))
        group = gpu.LocalGroup(slabs)
        for _ in range(steps):
            single.step(1)
            group.step(1)
        r1, u1 = single.macro()
        rg, ug = group.gather_macro()
        assert np.array_equal(rg, r1) and np.array_equal(ug, u1)
        assert abs(group.flux - single.flux) <= 1e-12 * max(abs(single.flux), 1e-30)
        assert single.count_nonfinite() == 0
    finally:
        for s in slabs + [single]:
            s.close()
