"""The f64 deep sweep's two-cell collide with its head in lock-step (iblb_device.h:relax_cells) and the
one-round default sweep width, against the one-step kernel (IBLB_SWEEP=0: fused_kernel, relax_cell on
one cell), bit for bit.

The two cells of a lane are rows r0 and r0 + 1, so a state that differs by row parity gives them very
different chains (density 1 against 1.2, velocities of opposite sign a decade apart): an element taken
from the other cell, or a temporary shared between the two, cannot cancel.  The reference of each
(shape, iteration count) is computed once and shared.
"""
import numpy as np
import pytest

import regimes as R

pytestmark = pytest.mark.gpu

DEEP_ENV = ("IBLB_SWEEP", "IBLB_SWEEP_DEPTH", "IBLB_DEEP_VS", "IBLB_DEEP_W", "IBLB_DEEP_BUILD", "IBLB_DEEP_BALANCE")
MODE_DEFAULT_F64 = 785  # nontemporal stores + wall split + preshift + LDS window (lbm_sweep_impl.h)
BODY = (1e-6, 3e-7)
_refs = {}


def parity_state(nx, ny, seed=11):
    """rho = 1 on even rows, 1.2 on odd rows; u random ~1e-3 on even rows, and on every odd row minus ten
    times the even row's below it (reference layout, j = y nx + x)."""
    from cuda_iblb_11_amd import workloads as W
    _, u = W.perturbed_state(nx, ny, seed)
    u = u.reshape(2, ny, nx).copy()
    rho = np.ones((ny, nx))
    rho[1::2] = 1.2
    u[:, 1::2] = -10.0 * u[:, 0:2 * (ny // 2):2]
    return rho.ravel(), u.ravel()


def _clean(monkeypatch):
    for name in DEEP_ENV:
        monkeypatch.delenv(name, raising=False)


def _one_step(P, monkeypatch, key, make, calls):
    """Populations and flux of the one-step path (shared, read-only)."""
    if key not in _refs:
        _clean(monkeypatch)
        monkeypatch.setenv("IBLB_SWEEP", "0")
        ref = make()
        for n in calls:
            ref.step(n)
        tm = ref.timing()
        assert tm["sweepk_launches"] == 0 and tm["sweep_launches"] == 0, tm
        f = ref.populations()
        f.setflags(write=False)
        _refs[key] = (f, ref.flux)
        ref.close()
        monkeypatch.delenv("IBLB_SWEEP")
    return _refs[key]


@pytest.mark.parametrize("balance", ["1", "0"])
@pytest.mark.parametrize("build", [None, "split,window"])
@pytest.mark.parametrize("depth", [6, 7])
@pytest.mark.parametrize("nx,ny", [(9, 171), (20, 170), (37, 300)])
def test_row_parity_contrast(gpu, monkeypatch, nx, ny, depth, build, balance):
    """One and two inner chunks, odd and even height, fewer columns than the walk's reach; depths 6 and 7;
    the default build and split,window; fixed and balanced sweeps.  Calls of 1 + 2K and 2K - 1 iterations
    (boot + two deep launches, then one of depth K - 1 and one of depth K)."""
    rho, u = parity_state(nx, ny)
    calls = [1 + 2 * depth, 2 * depth - 1]

    def make():
        lat = gpu.Lattice(nx, ny, R.TAUS["Re1"][0], R.TAUS["Re1"][1], precision="f64", body_force=BODY)
        lat.set_state(rho, u)
        lat.set_profiling(True)
        return lat

    f_ref, q_ref = _one_step(gpu, monkeypatch, ("parity", nx, ny, depth), make, calls)
    _clean(monkeypatch)
    monkeypatch.setenv("IBLB_SWEEP_DEPTH", str(depth))
    monkeypatch.setenv("IBLB_DEEP_BALANCE", balance)
    if build is not None:
        monkeypatch.setenv("IBLB_DEEP_BUILD", build)
    lat = make()
    for n in calls:
        lat.step(n)
    tm = lat.timing()
    f, q = lat.populations(), lat.flux
    lat.close()
    diff = float(np.max(np.abs(f - f_ref)))
    print("LOCKSTEP parity", nx, ny, depth, build, balance, "mode", tm["deep_mode"], "max|df|", diff,
          "dflux", abs(q - q_ref) / abs(q_ref))
    assert tm["sweepk_launches"] == 4 and tm["sweepk_depth"] == depth, tm
    assert tm["deep_mode"] == MODE_DEFAULT_F64 and tm["deep_vs"] == 2, tm
    assert np.array_equal(f, f_ref), diff
    assert abs(q - q_ref) <= 1e-13 * abs(q_ref), (q, q_ref)


@pytest.mark.parametrize("c", R.FULL, ids=R.ids(R.FULL))
def test_regime_sweep(gpu, monkeypatch, c):
    """Every relaxation pair, amplitude and body force of tests/regimes.py on 48 x 170 (the wall chunks and one inner chunk): one
    call of 1 + 2 * 7 iterations on the deep path against the one-step path."""
    nx, ny, calls = 48, 170, [1 + 2 * 7]
    rho, u = R.state(c, nx, ny)

    def make():
        lat = gpu.Lattice(nx, ny, c.tau, c.tau2, precision="f64", body_force=c.force)
        lat.set_state(rho, u)
        lat.set_profiling(True)
        return lat

    f_ref, q_ref = _one_step(gpu, monkeypatch, ("regime", c.id), make, calls)
    _clean(monkeypatch)
    lat = make()
    lat.step(calls[0])
    tm = lat.timing()
    f, q = lat.populations(), lat.flux
    lat.close()
    diff = float(np.max(np.abs(f - f_ref)))
    print("LOCKSTEP regime", c.id, "mode", tm["deep_mode"], "max|df|", diff, "dflux", abs(q - q_ref) / abs(q_ref))
    assert tm["sweepk_launches"] == 2 and tm["sweepk_depth"] == 7 and tm["deep_mode"] == MODE_DEFAULT_F64, tm
    assert np.array_equal(f, f_ref), diff
    assert abs(q - q_ref) <= 1e-13 * abs(q_ref), (q, q_ref)


@pytest.mark.parametrize("nx,ny", [(64, 300), (16, 4096)])
def test_one_round_sizing(gpu, monkeypatch, nx, ny):
    """The default sweep width (no IBLB_DEEP_W) with profiling on: a short lattice and a narrow one of M's
    height (35 inner chunks, sweeps narrower than the request) step 1 + 14 iterations as the one-step path
    does, in the 785 build."""
    rho, u = parity_state(nx, ny, seed=5)
    calls = [1 + 14]

    def make():
        lat = gpu.Lattice(nx, ny, R.TAUS["Re1"][0], R.TAUS["Re1"][1], precision="f64", body_force=BODY)
        lat.set_state(rho, u)
        lat.set_profiling(True)
        return lat

    f_ref, q_ref = _one_step(gpu, monkeypatch, ("sizing", nx, ny), make, calls)
    _clean(monkeypatch)
    lat = make()
    lat.step(calls[0])
    tm = lat.timing()
    f, q = lat.populations(), lat.flux
    lat.close()
    diff = float(np.max(np.abs(f - f_ref)))
    print("LOCKSTEP sizing", nx, ny, "mode", tm["deep_mode"], "max|df|", diff, "dflux", abs(q - q_ref) / abs(q_ref))
    assert tm["sweepk_launches"] == 2 and tm["sweepk_depth"] == 7, tm
    assert tm["deep_mode"] == MODE_DEFAULT_F64 and tm["deep_vs"] == 2 and tm["deep_waves_per_simd"] == 1, tm
    assert np.array_equal(f, f_ref), diff
    assert abs(q - q_ref) <= 1e-13 * abs(q_ref), (q, q_ref)
