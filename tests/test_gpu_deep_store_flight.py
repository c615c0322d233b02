"""The f64 window build's inner walks keep level K's stores in flight across the step boundary: every
step of an LDS-window walk issues nine stores, and the ones with nothing to write (a window-filling step,
a lane that owns no row, the walk's prologue) are addressed beyond the column resource's range, where
the buffer range check drops them (lbm_sweep_impl.h:store_in_flight).

A dropped store that landed after all would overwrite rows some other wave owns, and a store counted
as done too early would be read back half-written by the next launch; so every case compares the
populations bit for bit, and the flux to 1e-13 relative (per-wave atomics: the order varies), against
the one-step path (IBLB_SWEEP=0) or the lone slab, on the smallest shapes where that can show:

* 37 x 300 and 40 x 300: two inner chunks, whose ghost lanes lie over the owned rows of the other one and
  of the wall chunks; four deep launches back to back (the stores one launch leaves in flight, the
  loads of the next); 40 x 300 with sweeps of 16 columns too, fixed and balanced: forward and reverse
  walks side by side, whose filling steps address the neighbouring sweep's output columns;
* 9 x 171: one inner chunk and fewer columns than the walk's reach: the last steps reload columns, and
  every storing step is next to a filling one;
* the RCCL self ring's slab (the ghost-column build with the edge waves' hand-off, write-through
  stores in the edge waves) with profiling on, so that the done word is checked against the host's
  edge-wave count.

The reference of each (shape, depth) is computed once and shared, read-only.
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


def _make(gpu, nx, ny, precision="f64"):
    rho, u = parity_state(nx, ny)
    lat = gpu.Lattice(nx, ny, R.TAUS["Re1"][0], R.TAUS["Re1"][1], precision=precision, body_force=BODY)
    lat.set_state(rho, u)
    lat.set_profiling(True)
    return lat


def _one_step(gpu, monkeypatch, nx, ny, depth, calls):
    key = (nx, ny, depth)
    if key not in _refs:
        _clean(monkeypatch)
        monkeypatch.setenv("IBLB_SWEEP", "0")
        ref = _make(gpu, nx, ny)
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


def _deep_against_one_step(gpu, monkeypatch, nx, ny, depth, **env):
    calls = [1 + 2 * depth, 2 * depth - 1]  # boot + two deep launches, then depth K - 1 and depth K
    f_ref, q_ref = _one_step(gpu, monkeypatch, nx, ny, depth, calls)
    _clean(monkeypatch)
    monkeypatch.setenv("IBLB_SWEEP_DEPTH", str(depth))
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    lat = _make(gpu, nx, ny)
    for n in calls:
        lat.step(n)
    tm = lat.timing()
    f, q = lat.populations(), lat.flux
    lat.close()
    diff = float(np.max(np.abs(f - f_ref)))
    print("STOREFLIGHT", nx, ny, depth, env, "mode", tm["deep_mode"], "max|df|", diff, "dflux", abs(q - q_ref) / abs(q_ref))
    assert tm["sweepk_launches"] == 4 and tm["sweepk_depth"] == depth, tm
    assert tm["deep_mode"] == MODE_DEFAULT_F64 and tm["deep_vs"] == 2, tm
    assert np.array_equal(f, f_ref), diff
    assert abs(q - q_ref) <= 1e-13 * abs(q_ref), (q, q_ref)


@pytest.mark.parametrize("depth", [6, 7])
@pytest.mark.parametrize("nx,ny", [(37, 300), (40, 300)])
def test_two_inner_chunks(gpu, monkeypatch, nx, ny, depth):
    """Two inner chunks and the wall chunks, the default sweeps: four deep launches back to back."""
    _deep_against_one_step(gpu, monkeypatch, nx, ny, depth)


@pytest.mark.parametrize("balance", [0, 1])
@pytest.mark.parametrize("depth", [6, 7])
def test_sweeps_side_by_side(gpu, monkeypatch, depth, balance):
    """40 x 300 in sweeps of 16 columns, fixed and balanced: forward and reverse walks whose filling
    steps' dropped stores are addressed at their neighbours' output columns."""
    _deep_against_one_step(gpu, monkeypatch, 40, 300, depth, IBLB_DEEP_W=16, IBLB_DEEP_BALANCE=balance)


@pytest.mark.parametrize("depth", [6, 7])
def test_narrower_than_reach(gpu, monkeypatch, depth):
    """9 x 171: one inner chunk, fewer columns than the walk reaches."""
    _deep_against_one_step(gpu, monkeypatch, 9, 171, depth)


@pytest.mark.parametrize("precision,build", [("f64", (MODE_DEFAULT_F64, 2)), ("f32", (273, 1))])
def test_self_ring_slab(gpu, monkeypatch, precision, build):
    """The RCCL self ring's 64 x 300 slab (interior sweep of the ghost-column build, its edge waves handing
    their columns to the boundary sweeps) after 1, 7 and 13 iterations: equal to the lone slab bit for bit;
    profiling on, so the done word is checked against the host's edge-wave count at each call's end."""
    _clean(monkeypatch)
    nx, ny = 64, 300
    ref = _make(gpu, nx, ny, precision)
    monkeypatch.setenv("IBLB_RCCL_SELF", "1")
    ring = _make(gpu, nx, ny, precision)
    try:
        ring.attach_rccl(gpu.rccl_unique_id(), 1, 0)
        for n in (1, 7, 13):
            ref.step(n)
            ring.step(n)
            f1, f2 = ref.populations(), ring.populations()
            assert np.array_equal(f1, f2), (n, float(np.max(np.abs(f1 - f2))))
        tm = ring.timing()
        print("STOREFLIGHT ring", precision, "mode", tm["deep_mode"], tm["deep_vs"], "launches", tm["deep_launches"],
              tm["sweepk_launches"])
        assert tm["deep_launches"] == 3 and tm["deep_iterations"] == 20 and tm["sweepk_launches"] >= 3, tm
        assert (tm["deep_mode"], tm["deep_vs"]) == build, tm
        assert abs(ring.flux - ref.flux) <= 1e-13 * abs(ref.flux), (ring.flux, ref.flux)
    finally:
        ring.close()
        ref.close()
