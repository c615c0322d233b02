"""tests/scalar_source_ref.py, the numpy restatement of the scalar's rule with a source, pinned on the CPU: it reduces
to scalar_ref.substep, reaches the closed forms of a uniform source with decay and of steady conduction, and keeps the
budget the header states."""
import numpy as np
import pytest

import scalar_ref as S
import scalar_source_ref as Q

EPS = 2.0 ** -53


def random_state(rng, nx, ny):
    g = rng.uniform(0.1, 0.9, (5, ny, nx))
    ux, uy = rng.uniform(-0.05, 0.05, (2, ny, nx))
    return g, ux, uy


def test_equals_the_rule_without_a_source_when_every_term_is_zero():
    rng = np.random.default_rng(75)
    g, ux, uy = random_state(rng, 7, 5)
    walls = ((S.VALUE, 0.25), (S.NOFLUX, 0.0))
    got = Q.substep(g, ux, uy, 0.8, Q.Source(), walls)
    assert np.array_equal(got, S.substep(g, ux, uy, 0.8, walls))
    zeros = Q.Source(np.zeros((5, 7)), 0.0, (None, np.zeros(7)), (np.full(7, 0.25), None))
    assert np.array_equal(Q.substep(g, ux, uy, 0.8, zeros, walls), got)
    assert np.array_equal(Q.event(g, ux, uy, 0.8, 3, None, walls), S.event(g, ux, uy, 0.8, 3, walls))


def test_uniform_source_with_decay_follows_the_closed_form():
    nx, ny, tau, s, k, n = 3, 4, 0.9, 1e-3, 0.01, 200
    zero = np.zeros((ny, nx))
    g = S.equilibrium(zero, zero, zero)
    g = Q.event(g, zero, zero, tau, n, Q.Source(np.full((ny, nx), s), k))
    want = s / k * (1.0 - (1.0 - k) ** n)
    err = np.max(np.abs(S.concentration(g) - want)) / want
    print(f"uniform source: rel err {err:.3e}")
    assert err <= 1e-13  # n * 4 roundings * 2^-53 = 9e-14


def test_budget_over_one_substep():
    rng = np.random.default_rng(76)
    nx, ny = 7, 5
    g, ux, uy = random_state(rng, nx, ny)
    src = Q.Source(rng.uniform(-1e-2, 1e-2, (ny, nx)), 0.02,
                   (rng.uniform(-1e-2, 1e-2, nx), rng.uniform(-1e-2, 1e-2, nx)))
    assert np.any(src.wall_flux[0] < 0) and np.any(src.wall_flux[0] > 0)
    assert np.any(src.wall_flux[1] < 0) and np.any(src.wall_flux[1] > 0)
    C = S.concentration(g)
    C1 = S.concentration(Q.substep(g, ux, uy, 0.8, src))
    want = np.sum(Q.rate(C, src)) + np.sum(src.wall_flux[0] + src.wall_flux[1])
    got = np.sum(C1) - np.sum(C)
    bound = 64 * EPS * (np.sum(np.abs(C)) + np.sum(np.abs(C1)))
    print(f"budget: |got - want| {abs(got - want):.3e}, bound {bound:.3e}, sum C {np.sum(C):.3g}")
    assert want != 0.0 and abs(got - want) <= bound


@pytest.mark.parametrize("tau", [0.8, 1.0, 1.5])
def test_steady_conduction_between_an_influx_and_a_value_wall(tau):
    nx, ny, q, n = 3, 8, 1e-3, 20000
    zero = np.zeros((ny, nx))
    walls = ((S.NOFLUX, 0.0), (S.VALUE, 0.0))
    g = S.equilibrium(zero, zero, zero)
    g = Q.event(g, zero, zero, tau, n, Q.Source(wall_flux=(np.full(nx, q), None)), walls)
    D = (tau - 0.5) / 3.0
    want = (q / D) * (ny - 0.5 - np.arange(ny))[:, None] * np.ones((ny, nx))
    err = np.max(np.abs(S.concentration(g) - want) / want)
    print(f"conduction tau {tau}: rel err {err:.3e}")
    assert err <= 1e-12
