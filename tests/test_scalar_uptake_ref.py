"""tests/scalar_uptake_ref.py, the numpy restatement of the scalar's rule with an uptake, pinned on the CPU: it
reduces to the rules without one, reaches the _VALUE wall at 0.0 for a huge rate, is exact for the steady state between
a reactive and a _VALUE wall, keeps the budget the header states, and counts `stride` substeps per event."""
import math

import numpy as np
import pytest

import scalar_ref as S
import scalar_source_ref as Q
import scalar_uptake_ref as U

EPS = 2.0 ** -53
SIZES = [(20, 18), (37, 23), (16, 300)]


def random_state(rng, nx, ny):
    g = rng.uniform(0.1, 0.9, (5, ny, nx))
    ux, uy = rng.uniform(-0.05, 0.05, (2, ny, nx))
    return g, ux, uy


def mixed_rates(rng, nx):
    """Rates with entries 0, 1/3 and 50 among random ones."""
    r = rng.uniform(0.0, 2.0, nx)
    r[[0, nx // 2, nx - 1]] = (0.0, 1.0 / 3.0, 50.0)
    return r


# ---- 1. zero rates -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ny", [5, 1])
def test_zero_rates_equal_the_rules_without_an_uptake(ny):
    rng = np.random.default_rng(81)
    nx = 7
    g, ux, uy = random_state(rng, nx, ny)
    walls = ((S.VALUE, 0.25), (S.NOFLUX, 0.0))
    src = Q.Source(rng.uniform(-1e-2, 1e-2, (ny, nx)), 0.02, (None, rng.uniform(-1e-2, 1e-2, nx)),
                   (rng.uniform(0.1, 0.4, nx), None))
    for up in (U.Uptake(), U.Uptake((None, np.zeros(nx)))):
        got, _ = U.substep(g, ux, uy, 0.8, up, U.Sums(nx), None, walls)
        assert np.array_equal(got, S.substep(g, ux, uy, 0.8, walls))
        got, _ = U.substep(g, ux, uy, 0.8, up, U.Sums(nx), src, walls)
        assert np.array_equal(got, Q.substep(g, ux, uy, 0.8, src, walls))
    # between no-flux walls without a source nothing crosses: the totals are 0
    for up in (U.Uptake(), U.Uptake((np.zeros(nx), np.zeros(nx)))):
        got, sums = U.event(g, ux, uy, 0.8, 3, up, U.Sums(nx))
        assert np.array_equal(got, S.event(g, ux, uy, 0.8, 3))
        assert np.array_equal(sums.total, np.zeros((2, nx))) and np.array_equal(sums.last, np.zeros((2, nx)))
        assert sums.substeps == 3
    # at the _VALUE wall the accumulators hold what iblb_get_scalar_wall_flux states for that substep
    got, sums = U.substep(g, ux, uy, 0.8, U.Uptake(), U.Sums(nx), src, walls)
    want = Q.wall_flux(got, src, walls)
    assert np.allclose(sums.last[0], want[0], rtol=0, atol=8 * EPS) and np.array_equal(sums.last[1], want[1])
    # no uptake: the event of the rule in force, the sums untouched
    sums0 = U.Sums(nx)
    got, sums = U.event(g, ux, uy, 0.8, 3, None, sums0, src, walls)
    assert sums is sums0 and np.array_equal(got, Q.event(g, ux, uy, 0.8, 3, src, walls))


# ---- 2. a huge rate ------------------------------------------------------------------------------------------

def test_a_huge_rate_is_the_value_wall_at_zero():
    rng = np.random.default_rng(82)
    nx, ny = 7, 5
    g, ux, uy = random_state(rng, nx, ny)
    up = U.Uptake((np.full(nx, 1e300), None))
    assert np.array_equal(up.coefficient(0, nx), np.full(nx, 2.0))
    assert np.array_equal(U.Uptake((np.full(nx, 1.7e308), None)).coefficient(0, nx), np.full(nx, 2.0))  # 3 k overflows
    got, sums = U.event(g, ux, uy, 0.8, 4, up, U.Sums(nx))
    walls = ((S.VALUE, 0.0), (S.NOFLUX, 0.0))
    assert np.array_equal(got, S.event(g, ux, uy, 0.8, 4, walls))
    assert np.all(sums.total[0] < 0) and np.array_equal(sums.total[1], np.zeros(nx))


# ---- 3. the steady state -------------------------------------------------------------------------------------

class NaiveUptake(U.Uptake):
    """a = 6 k: the loss taken as k times the cell's own population, not k C at the wall."""

    def coefficient(self, k, nx):
        return np.zeros(nx) if self.rate[k] is None else 6.0 * np.asarray(self.rate[k], dtype=np.float64)


def steady_errors(tau, k, up_type=U.Uptake, ny=8, nx=1):
    """From C = 1 at rest between a reactive wall below and a _VALUE wall at 1.0 above: (max |C - analytic|, relative
    error of the loss per substep against k C_w).  Substeps: the slowest mode decays about as D (pi / (2 ny))^2 per
    substep at small k (a quarter wave between the no-flux-like wall and the value wall; faster at larger k), and
    exp(-40) = 4e-18 of an O(1) start is below the last place."""
    D = (tau - 0.5) / 3.0
    n = math.ceil(40.0 / (D * (math.pi / (2 * ny)) ** 2))
    zero = np.zeros((ny, nx))
    walls = ((S.NOFLUX, 0.0), (S.VALUE, 1.0))
    g = S.equilibrium(np.ones((ny, nx)), zero, zero)
    g, sums = U.event(g, zero, zero, tau, n, up_type((np.full(nx, k), None)), U.Sums(nx), None, walls)
    cw = D / (D + k * ny)
    want = cw + (1.0 - cw) * (np.arange(ny) + 0.5)[:, None] / ny * np.ones((ny, nx))
    err_c = np.max(np.abs(S.concentration(g) - want))
    err_q = np.max(np.abs(-sums.last[0] - k * cw)) / (k * cw)
    # in the steady state what leaves below enters above
    assert np.allclose(sums.last[1], -sums.last[0], rtol=1e-11, atol=0)
    return n, err_c, err_q


@pytest.mark.parametrize("k", [0.01, 0.1, 1.0 / 3.0, 2.0, 50.0])
@pytest.mark.parametrize("tau", [0.6, 0.8, 1.0, 1.5])
def test_the_steady_state_is_exact(tau, k):
    """Within 1e-12: the reference's own error here is <= 6e-14, and the margin leaves room for another substep
    count."""
    n, err_c, err_q = steady_errors(tau, k)
    print(f"tau {tau} k {k:.4g}: {n} substeps, profile err {err_c:.3e}, flux rel err {err_q:.3e}")
    assert err_c <= 1e-12 and err_q <= 1e-12


def test_the_naive_coefficient_misses_the_steady_state():
    n, err_c, err_q = steady_errors(1.0, 0.1, NaiveUptake)
    print(f"a = 6 k: profile err {err_c:.3e}, flux rel err {err_q:.3e}")
    assert err_c > 1e-3 and err_q > 1e-3


# ---- 4. the budget -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", SIZES)
def test_budget_over_21_substeps(nx, ny):
    rng = np.random.default_rng(nx * 31 + ny)
    g, ux, uy = random_state(rng, nx, ny)
    up = U.Uptake((mixed_rates(rng, nx), mixed_rates(rng, nx)))
    n_sub = 21
    C0 = S.concentration(g)
    g1, sums = U.event(g, ux, uy, 0.8, n_sub, up, U.Sums(nx))
    C1 = S.concentration(g1)
    got = np.sum(C1) - np.sum(C0)
    want = np.sum(sums.total[0] + sums.total[1])
    bound = U.budget_bound(nx * ny, n_sub, nx, max(np.sum(np.abs(C0)), np.sum(np.abs(C1))))
    print(f"{nx} x {ny}: d sum(C) {got:.6e}, totals {want:.6e}, |diff| {abs(got - want):.3e}, bound {bound:.3e}")
    assert sums.substeps == n_sub and want < 0.0
    assert abs(got - want) <= bound
    # one wall's accumulator left out misses by orders of magnitude
    assert abs(got - np.sum(sums.total[0])) > 1e6 * bound and abs(got - np.sum(sums.total[1])) > 1e6 * bound


# ---- 5. substeps count `stride` per event --------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 5, 7])
def test_substeps_count_stride_per_event(stride):
    rng = np.random.default_rng(83)
    nx, ny = 6, 4
    g, ux, uy = random_state(rng, nx, ny)
    up = U.Uptake((mixed_rates(rng, nx), None))
    sums, events = U.Sums(nx), 0
    for n, due in S.pieces([9, 11], 2, scalar=(2, stride)):
        if due["scalar"]:
            g, sums = U.event(g, ux, uy, 0.8, stride, up, sums)
            events += 1
            assert sums.substeps == stride * events
    assert events == 20 // stride
