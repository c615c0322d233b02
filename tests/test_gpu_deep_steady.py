"""The f64 window build's inner walks run their steps in ranges (lbm_sweep_impl.h:step_ranges): the
window-filling steps [0, 2(K-1)) and the K steps at which some level stands on the flux column go through
the general iteration, every other step through the branch-free STEADY one.  The step counter, the column
pointers, the loaded column and the windows pass from one range to the next, so a seam in the wrong place
computes a level on a window that is not filled, skips or repeats a column, or misses a level's flux.

Every case compares a deep run with the one-step path (IBLB_SWEEP=0) over calls of 1 + 2K and 2K - 1
iterations (boot + two deep launches, then one of depth K - 1 and one of depth K; depth 3 has no K - 1
launch: a deep launch and a two-iteration sweep): populations bit for bit,
flux to 1e-13 relative (per-wave atomics: the order varies), build and launch count asserted.

* range seams, depths 3-7 on 40 x 300 (two inner chunks and the wall chunks): sweeps of one column (level-1
  columns 2(K-1) + 1: exactly one steady step), of two, and of 16 fixed and balanced (forward and reverse
  walks side by side, the last sweep 8 wide);
* 9 x 171, depths 6 and 7: one inner chunk, fewer columns than the walk's reach (reloaded columns);
* the flux steps, depths 6 and 7 on 40 x 300 in fixed sweeps of 16: the flux column the first and last
  output of a forward sweep (0, 15) and of a reverse one (16, 31), where the flux range overlaps the filling
  range or reaches the walk's last step; mid-sweep (24), between two steady ranges; nx - 1 (the narrow last
  sweep, the periodic edge); the default nx - 5; and one-column sweeps, the flux column in one of them;
* the RCCL self ring's 64 x 300 slab (the ghost-column build; write-through walks in the edge waves) against
  the lone slab after 1, 7 and 13 iterations, the flux column in an edge sweep of the interior (10) and in
  its middle (32), profiling on so the done word is checked against the host's edge-wave count.  (The
  ghost-column build keeps the single-loop walk, step_ranges excludes it: the lone slab it is compared
  with runs the ranges, the ring must equal it.)

The reference of each (shape, depth, flux column) is computed once and shared, read-only.
"""
import numpy as np
import pytest

import regimes as R
from test_gpu_deep_lockstep import DEEP_ENV, MODE_DEFAULT_F64, parity_state

pytestmark = pytest.mark.gpu

BODY = (1e-6, 3e-7)
_refs = {}


def _clean(monkeypatch):
    for name in DEEP_ENV + ("IBLB_RCCL_SELF",):
        monkeypatch.delenv(name, raising=False)


def _make(gpu, nx, ny, flux_column=None):
    rho, u = parity_state(nx, ny)
    lat = gpu.Lattice(nx, ny, R.TAUS["Re1"][0], R.TAUS["Re1"][1], precision="f64", body_force=BODY,
                      flux_column=flux_column)
    lat.set_state(rho, u)
    lat.set_profiling(True)
    return lat


def _one_step(gpu, monkeypatch, nx, ny, depth, flux_column, calls):
    key = (nx, ny, depth, flux_column)
    if key not in _refs:
        _clean(monkeypatch)
        monkeypatch.setenv("IBLB_SWEEP", "0")
        ref = _make(gpu, nx, ny, flux_column)
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


def _deep_against_one_step(gpu, monkeypatch, nx, ny, depth, flux_column=None, **env):
    calls = [1 + 2 * depth, 2 * depth - 1]
    f_ref, q_ref = _one_step(gpu, monkeypatch, nx, ny, depth, flux_column, calls)
    _clean(monkeypatch)
    monkeypatch.setenv("IBLB_SWEEP_DEPTH", str(depth))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    lat = _make(gpu, nx, ny, flux_column)
    for n in calls:
        lat.step(n)
    tm = lat.timing()
    f, q = lat.populations(), lat.flux
    lat.close()
    diff = float(np.max(np.abs(f - f_ref)))
    print("STEADY", nx, ny, depth, "flux column", flux_column, env, "mode", tm["deep_mode"], tm["deep_vs"], "launches",
          tm["sweepk_launches"], tm["sweepk_depth"], "max|df|", diff, "dflux", abs(q - q_ref) / abs(q_ref))
    assert q_ref != 0.0
    # depth 3 mixes no K - 1: its second call is one deep launch and one two-iteration sweep
    assert tm["sweepk_launches"] == (4 if depth >= 4 else 3) and tm["sweepk_depth"] == depth, tm
    assert tm["sweep_launches"] == (0 if depth >= 4 else 1), tm
    assert tm["deep_mode"] == MODE_DEFAULT_F64 and tm["deep_vs"] == 2, tm
    assert np.array_equal(f, f_ref), diff
    assert abs(q - q_ref) <= 1e-13 * abs(q_ref), (q, q_ref)


@pytest.mark.parametrize("w", [1, 2])
@pytest.mark.parametrize("depth", [3, 4, 5, 6, 7])
def test_seams_narrow_sweeps(gpu, monkeypatch, depth, w):
    """Fixed sweeps of one column (exactly one steady step after the filling steps) and of two."""
    _deep_against_one_step(gpu, monkeypatch, 40, 300, depth, IBLB_DEEP_W=w, IBLB_DEEP_BALANCE=0)


@pytest.mark.parametrize("balance", [0, 1])
@pytest.mark.parametrize("depth", [3, 4, 5, 6, 7])
def test_seams_side_by_side(gpu, monkeypatch, depth, balance):
    """Sweeps of 16 columns, fixed (the last one 8 wide) and balanced: forward and reverse walks side by side."""
    _deep_against_one_step(gpu, monkeypatch, 40, 300, depth, IBLB_DEEP_W=16, IBLB_DEEP_BALANCE=balance)


@pytest.mark.parametrize("depth", [6, 7])
def test_no_steady_step(gpu, monkeypatch, depth):
    """9 x 171: one inner chunk, fewer columns than the walk's reach, so the walks load columns they hold
    already; the balanced default gives one-column sweeps, and the one that holds the flux column (4) has
    no steady step at all."""
    _deep_against_one_step(gpu, monkeypatch, 9, 171, depth)


@pytest.mark.parametrize("c", [0, 15, 16, 31, 24, 39, None], ids=lambda c: "default" if c is None else f"c{c}")
@pytest.mark.parametrize("depth", [6, 7])
def test_flux_steps(gpu, monkeypatch, depth, c):
    """The flux column at the ends of a forward sweep [0, 16) and of a reverse one [16, 32), inside one, at
    the periodic edge in the narrow last sweep [32, 40), and at the default nx - 5."""
    _deep_against_one_step(gpu, monkeypatch, 40, 300, depth, flux_column=c, IBLB_DEEP_W=16, IBLB_DEEP_BALANCE=0)


@pytest.mark.parametrize("depth", [6, 7])
def test_flux_in_one_column_sweep(gpu, monkeypatch, depth):
    """One-column sweeps: the flux steps are the last K of the walk's 2(K-1) + 1, K - 1 of them filling steps."""
    _deep_against_one_step(gpu, monkeypatch, 40, 300, depth, flux_column=21, IBLB_DEEP_W=1, IBLB_DEEP_BALANCE=0)


@pytest.mark.parametrize("c", [10, 32], ids=["edge", "interior"])
def test_self_ring_slab_flux(gpu, monkeypatch, c):
    """The self ring's slab: the interior sweep's outputs are columns [7, 57), its edge waves the ones with
    outputs below 16 or above 48 (write-through walks).  Equal to the lone slab bit for bit."""
    _clean(monkeypatch)
    nx, ny = 64, 300
    ref = _make(gpu, nx, ny, c)
    monkeypatch.setenv("IBLB_RCCL_SELF", "1")
    ring = _make(gpu, nx, ny, c)
    try:
        ring.attach_rccl(gpu.rccl_unique_id(), 1, 0)
        for n in (1, 7, 13):
            ref.step(n)
            ring.step(n)
            f1, f2 = ref.populations(), ring.populations()
            assert np.array_equal(f1, f2), (n, float(np.max(np.abs(f1 - f2))))
        tm = ring.timing()
        print("STEADY ring flux column", c, "mode", tm["deep_mode"], tm["deep_vs"], "launches", tm["deep_launches"],
              tm["sweepk_launches"], "dflux", abs(ring.flux - ref.flux) / abs(ref.flux))
        assert tm["deep_launches"] == 3 and tm["deep_iterations"] == 20 and tm["sweepk_launches"] >= 3, tm
        assert (tm["deep_mode"], tm["deep_vs"]) == (MODE_DEFAULT_F64, 2), tm
        assert ref.flux != 0.0
        assert abs(ring.flux - ref.flux) <= 1e-13 * abs(ref.flux), (ring.flux, ref.flux)
    finally:
        ring.close()
        ref.close()
