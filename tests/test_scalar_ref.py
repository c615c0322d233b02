"""tests/scalar_ref.py on the CPU: the restated rule of iblb_set_scalar conserves the scalar between no-flux
walls, diffuses at D = (tau - 0.5)/3, holds the linear profile between two value walls, and its planner cuts
calls as average_ref.pieces does for two event sets.  The GPU tests (tests/test_gpu_scalar.py) compare the
device with this restatement bit for bit; these tests show that the restatement is the scheme it claims to be.
"""
import math

import numpy as np
import pytest

import average_ref as A
import scalar_ref as S


def seeded_velocity(nx, ny, amplitude, seed=5):
    rng = np.random.default_rng(seed)
    return amplitude * rng.uniform(-1.0, 1.0, (ny, nx)), amplitude * rng.uniform(-1.0, 1.0, (ny, nx))


@pytest.mark.parametrize("tau", [0.52, 0.8, 1.0, 1.7])
def test_no_flux_walls_conserve_the_scalar(tau):
    nx, ny = 37, 23
    ux, uy = seeded_velocity(nx, ny, 0.05)
    C0 = np.random.default_rng(6).uniform(0.0, 1.0, (ny, nx))
    g = S.equilibrium(C0, ux, uy)
    total0 = math.fsum(S.concentration(g).ravel())
    assert np.array_equal(S.concentration(g), S.concentration(S.equilibrium(C0, ux, uy)))
    drift = 0.0
    for k in range(400):
        g = S.substep(g, ux, uy, tau)
        if k % 50 == 49:
            drift = max(drift, abs(math.fsum(S.concentration(g).ravel()) - total0) / total0)
    print(f"tau {tau}: relative drift of sum(C) over 400 substeps {drift:.3e}")
    assert np.all(np.isfinite(g))
    assert not np.array_equal(S.concentration(g), C0)
    assert drift <= 1e-12


@pytest.mark.parametrize("tau", [0.6, 1.0, 1.7])
def test_a_sine_decays_at_the_diffusivity(tau):
    nx, ny, n = 64, 8, 300
    k = 2.0 * math.pi / nx
    mode = np.sin(k * np.arange(nx))
    C0 = np.tile(1.0 + 0.1 * mode, (ny, 1))
    zero = np.zeros((ny, nx))
    g = S.equilibrium(C0, zero, zero)
    amp = lambda g: float(np.mean(S.concentration(g) @ mode) * 2.0 / nx)
    a0 = amp(g)
    for _ in range(n):
        g = S.substep(g, zero, zero, tau)
    rate = -math.log(amp(g) / a0) / n
    D = (tau - 0.5) / 3.0
    print(f"tau {tau}: decay rate / (D k^2) = {rate / (D * k * k):.4f}")
    assert abs(a0 - 0.1) < 1e-12
    assert abs(rate / (D * k * k) - 1.0) <= 0.02


def test_value_walls_hold_the_linear_profile():
    nx, ny = 4, 17
    zero = np.zeros((ny, nx))
    walls = ((S.VALUE, 0.0), (S.VALUE, 1.0))
    g = S.equilibrium(np.full((ny, nx), 0.5), zero, zero)
    for _ in range(20000):
        g = S.substep(g, zero, zero, 0.9, walls)
    C = S.concentration(g)
    want = ((np.arange(ny) + 0.5) / ny)[:, None]
    err = float(np.max(np.abs(C - want)))
    print(f"value walls 0 and 1, tau 0.9, 20000 substeps: max |C(y) - (y + 0.5)/17| = {err:.3e}")
    assert err <= 1e-12


def test_substep_moves_each_population_one_cell_and_reflects_at_the_walls():
    """tau = 1 and u = 0: p_i = geq_i = w_i C, so a single marked cell shows where every direction goes."""
    nx, ny = 5, 4
    zero = np.zeros((ny, nx))
    for (x, y) in [(2, 1), (0, 0), (4, 3)]:
        C = np.zeros((ny, nx))
        C[y, x] = 6.0
        out = S.substep(S.equilibrium(C, zero, zero), zero, zero, 1.0)
        want = np.zeros((5, ny, nx))
        want[0, y, x] = 2.0
        want[1, y, (x + 1) % nx] = 1.0
        want[2, y, (x - 1) % nx] = 1.0
        if y + 1 < ny:
            want[3, y + 1, x] = 1.0
        else:
            want[4, y, x] = 1.0
        if y > 0:
            want[4, y - 1, x] = 1.0
        else:
            want[3, y, x] = 1.0
        assert np.array_equal(out, want), (x, y)
    # a value wall: the reflected population is (2 w1) value - p
    C = np.zeros((ny, nx))
    C[0, 1] = 6.0
    out = S.substep(S.equilibrium(C, zero, zero), zero, zero, 1.0, ((S.VALUE, 0.75), (S.VALUE, -3.0)))
    assert out[3, 0, 1] == (2.0 * S.W1) * 0.75 - 1.0 and out[3, 0, 0] == (2.0 * S.W1) * 0.75
    assert np.all(out[4, ny - 1] == (2.0 * S.W1) * -3.0)


def test_a_nonfinite_value_spreads():
    nx, ny = 6, 5
    zero = np.zeros((ny, nx))
    C = np.ones((ny, nx))
    C[2, 3] = np.nan
    g = S.event(S.equilibrium(C, zero, zero), zero, zero, 0.8, 2)
    bad = ~np.isfinite(S.concentration(g))
    assert bad[2, 3] and bad[2, 5] and bad[0, 3] and bad[3, 4] and not bad[2, 0] and bad.sum() == 13


def test_the_planner_agrees_with_the_two_set_planner_and_takes_a_third_set():
    for calls, t, tr, av in [([3, 4, 13], 2, (2, 3), (2, 5)), ([17], 0, (0, 3), (0, 4)), ([5, 5], 7, None, (3, 4)),
                             ([6], 0, None, None)]:
        got = S.pieces(calls, t, tracers=tr, average=av)
        assert [(n, d["tracers"], d["average"]) for n, d in got] == A.pieces(calls, t, tracers=tr, average=av)
    plan = S.pieces([20], 0, scalar=(0, 5), tracers=(0, 3), average=(0, 4))
    ends = np.cumsum([n for n, _ in plan])
    assert list(ends) == [3, 4, 5, 6, 8, 9, 10, 12, 15, 16, 18, 20]
    for end, (_, due) in zip(ends, plan):
        assert due == {"scalar": end % 5 == 0, "tracers": end % 3 == 0, "average": end % 4 == 0}
    # events count from t0, not from t: set at 2 with stride 5, the state at 4, the first event after iteration 7
    assert S.pieces([10], 4, scalar=(2, 5)) == [(3, {"scalar": True}), (5, {"scalar": True}), (2, {"scalar": False})]
    with pytest.raises(ValueError):
        S.pieces([1], 0, scalar=(0, 0))
