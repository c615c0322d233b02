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
# bounds with IB: the band tests' (test_gpu_fused.py::test_ib_band_cycle_matches_oracle)
IB_TOL = {"f64": {"fields": 1e-10, "force": 1e-9, "F_s": 1e-5, "flux": 1e-9},
          "f32": {"fields": TOL32, "force": 1e-3, "F_s": 1e-2, "flux": 1e-4}}


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
def _check_ib(test, lat, sim, c, precision, **extra):
    e = R.field_errors(*lat.macro(), sim.rho, sim.u)
    e_force = R.rel(lat.force(), sim.force)
    e_fs = R.rel(lat.lagrangian_force(), sim.F_s)
    e_q = abs(lat.flux - sim.flux) / max(abs(sim.flux), 1e-30)
    _report(test, c, precision, **e, force=e_force, F_s=e_fs, flux=e_q, **extra)
    tol = IB_TOL[precision]
    assert max(e.values()) <= tol["fields"], e
    assert e_force <= tol["force"] and e_fs <= tol["F_s"] and e_q <= tol["flux"], (e_force, e_fs, e_q)
    assert lat.count_nonfinite() == 0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", R.CORNERS, ids=R.ids(R.CORNERS))
def test_ib_one_step_regimes(gpu, oracle, c, precision):
    """The IB one-step path, 64 x 192 over 30 iterations, points given every iteration: the moving points
    of test_ib_edges_and_epsilon (at x ~ 0 and x ~ XDIM, masked ones) at the case's IB speed."""
    nx, ny, steps = 64, 192, 30
    pts = R.edge_points(nx, c.ib_amp)
    rho, u = R.state(c, nx, ny)
    sim = oracle.Simulation(nx, ny, c.tau, c.tau2, rho=rho, u=u, body_force=c.force)
    lat = _lattice(gpu, c, nx, ny, precision, max_points=4096)
    try:
        lat.set_state(rho, u)
        for it in range(steps):
            sim.set_lagrangian(*pts(it))
            lat.set_lagrangian(*pts(it))
            sim.step(1)
            lat.step(1)
        _check_ib("ib_one_step", lat, sim, c, precision)
    finally:
        lat.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c", R.CORNERS, ids=R.ids(R.CORNERS))
def test_ib_band_cycle_regimes(gpu, oracle, c, precision, monkeypatch):
    """The IB band cycle, 256 x 128 with a standing 40-point line at the case's IB speed: one call of
    3K + 2 iterations under IBLB_IB_BAND=1 against the oracle, and in f64 against the same call on the
    one-step path (IBLB_IB_BAND=0) within 1e-10 (equal up to the arrival order of the spread atomics)."""
    nx, ny, steps = 256, 128, 3 * K + 2
    pts = R.line(100.0, 40, amp=c.ib_amp)
    rho, u = R.state(c, nx, ny, 11)
    sim = oracle.Simulation(nx, ny, c.tau, c.tau2, rho=rho, u=u, body_force=c.force)
    sim.set_lagrangian(*pts)
    sim.step(steps)
    out = {}
    for band in ("1", "0") if precision == "f64" else ("1",):
        monkeypatch.setenv("IBLB_IB_BAND", band)
        lat = _lattice(gpu, c, nx, ny, precision, max_points=4096)
        try:
            lat.set_state(rho, u)
            lat.set_lagrangian(*pts)
            lat.set_profiling(True)
            lat.step(steps)
            n_deep = lat.timing()["sweepk_launches"]
            assert n_deep >= 3 if band == "1" else n_deep == 0, lat.timing()
            _check_ib("ib_band" + band, lat, sim, c, precision, sweepk_launches=n_deep)
            out[band] = (*lat.macro(), lat.force())
        finally:
            lat.close()
    if precision == "f64":
        d = [R.rel(a, b) for a, b in zip(out["1"], out["0"])]
        _report("ib_band_vs_one_step", c, precision, rho=d[0], u=d[1], force=d[2])
        assert max(d) <= 1e-10, d


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
