"""tests/scalar_ends_ref.py, the numpy restatement of the scalar's rule with open ends in x, pinned on the CPU: its
streaming map is a bijection at every size down to one column, without ends it is the existing restatements, it keeps
the linear profile between two value ends with the flux D/16, lets a blob leave through an outflow end where the
periodic twin keeps it, keeps the budget the header states, and tells two seeded mistakes apart.

Narrow lattices (1, 2, 3 columns) are covered here only: the GPU suite's lattices have 16 columns or more."""
import itertools

import numpy as np
import pytest

import scalar_ref as S
import scalar_source_ref as Q
import scalar_uptake_ref as U
import scalar_ends_ref as E

EPS = 2.0 ** -53
KIND_PAIRS = list(itertools.product(("noflux", "value", "outflow"), repeat=2))


def random_state(rng, nx, ny):
    g = rng.uniform(0.1, 0.9, (5, ny, nx))
    ux, uy = rng.uniform(-0.05, 0.05, (2, ny, nx))
    return g, ux, uy


class NeighbourOutflow(E.Ends):
    """Seeded mistake: an outflow end takes the inner neighbour's relaxed population, not the cell's own."""

    def received(self, k, p, ny):
        new, q = super().received(k, p, ny)
        if self.kind[k] == E.OUTFLOW:
            col, inward = ((1, 1), (-2, 2))[k]
            new = p[inward][:, col]
        return new, q


class FlippedValue(E.Ends):
    """Seeded mistake: a value end with the sign of q flipped, (2 w1) v + q."""

    def received(self, k, p, ny):
        new, q = super().received(k, p, ny)
        if self.kind[k] == E.VALUE:
            new = (2.0 * S.W1) * self.v(k, ny) + q
        return new, q


# ---- 1. the bijection ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ny", [2, 5])
@pytest.mark.parametrize("nx", [1, 2, 3, 16])
def test_every_output_element_has_one_writer(nx, ny):
    rng = np.random.default_rng(nx * 17 + ny)
    g, ux, uy = random_state(rng, nx, ny)
    src = Q.Source(rng.uniform(-1e-2, 1e-2, (ny, nx)), 0.02, (rng.uniform(-1e-2, 1e-2, nx), None))
    up = U.Uptake((rng.uniform(0.0, 2.0, nx), None))
    for kind in KIND_PAIRS:
        ends = E.Ends(kind, (0.7, 0.2), (rng.uniform(0.0, 1.0, ny), None) if kind[0] == "value" else (None, None))
        for kw in (dict(), dict(src=src), dict(up=up, up_sums=U.Sums(nx)), dict(up=up, up_sums=U.Sums(nx), src=src)):
            count = np.zeros(g.shape, dtype=np.int64)
            out, sums, _ = E.substep(g, ux, uy, 0.8, ends, E.Sums(ny), count=count, **kw)
            assert np.array_equal(count, np.ones_like(count)), (kind, sorted(kw))
            assert np.all(np.isfinite(out)), (kind, sorted(kw))  # the output starts as NaN: nothing is left out
            assert sums.substeps == 1 and sums.total.shape == sums.last.shape == (2, ny)


# ---- 2. without ends: the existing restatements; with them only the end columns' planes 1 and 2 change --------

def test_without_ends_the_event_is_the_rule_in_force():
    rng = np.random.default_rng(91)
    nx, ny = 7, 5
    g, ux, uy = random_state(rng, nx, ny)
    walls = ((S.VALUE, 0.25), (S.NOFLUX, 0.0))
    src = Q.Source(rng.uniform(-1e-2, 1e-2, (ny, nx)), 0.02)
    up = U.Uptake((None, rng.uniform(0.0, 2.0, nx)))
    sums0 = E.Sums(ny)
    got, sums, us = E.event(g, ux, uy, 0.8, 3, None, sums0, walls=walls)
    assert sums is sums0 and us is None and np.array_equal(got, S.event(g, ux, uy, 0.8, 3, walls))
    got, sums, us = E.event(g, ux, uy, 0.8, 3, None, sums0, src=src, walls=walls)
    assert sums is sums0 and us is None and np.array_equal(got, Q.event(g, ux, uy, 0.8, 3, src, walls))
    got, sums, us = E.event(g, ux, uy, 0.8, 3, None, sums0, up, U.Sums(nx), src, walls)
    want, want_us = U.event(g, ux, uy, 0.8, 3, up, U.Sums(nx), src, walls)
    assert sums is sums0 and np.array_equal(got, want) and np.array_equal(us.total, want_us.total)


@pytest.mark.parametrize("kind", KIND_PAIRS)
def test_one_substep_changes_only_the_end_columns(kind):
    rng = np.random.default_rng(92)
    nx, ny = 7, 5
    g, ux, uy = random_state(rng, nx, ny)
    walls = ((S.VALUE, 0.25), (S.NOFLUX, 0.0))
    src = Q.Source(rng.uniform(-1e-2, 1e-2, (ny, nx)), 0.02)
    up = U.Uptake((None, rng.uniform(0.0, 2.0, nx)))
    ends = E.Ends(kind, (0.7, 0.2))
    got, sums, us = E.substep(g, ux, uy, 0.8, ends, E.Sums(ny), up, U.Sums(nx), src, walls)
    want, want_us = U.substep(g, ux, uy, 0.8, up, U.Sums(nx), src, walls)
    same = np.ones(g.shape, dtype=bool)
    same[1, :, 0] = same[2, :, -1] = False
    assert np.array_equal(got[same], want[same])
    assert np.array_equal(us.total, want_us.total) and np.array_equal(us.last, want_us.last)
    # the rule, end by end, from the relaxed populations
    p = U.relaxed(g, ux, uy, 0.8, src)
    for k, (q, own, new) in enumerate(((p[2][:, 0], p[1][:, 0], got[1][:, 0]), (p[1][:, -1], p[2][:, -1], got[2][:, -1]))):
        want_new = {"noflux": q, "value": (2.0 * S.W1) * np.full(ny, ends.value[k]) - q, "outflow": own}[kind[k]]
        assert np.array_equal(new, want_new), k
        assert np.array_equal(sums.last[k], want_new - q) and np.array_equal(sums.total[k], 0.0 + (want_new - q))
    # what the wrapped populations were is gone: p_1(nx - 1, y) and p_2(0, y) reach no other column
    if kind[0] != "noflux":
        assert not np.any(got[1][:, 0] == want[1][:, 0])


def outflow_copies_what_the_neighbour_receives(ends_type):
    """Under _OUTFLOW g_1'(0, y) == g_1'(1, y) and g_2'(nx - 1, y) == g_2'(nx - 2, y), bit for bit."""
    rng = np.random.default_rng(93)
    nx, ny = 6, 4
    g, ux, uy = random_state(rng, nx, ny)
    out, _, _ = E.substep(g, ux, uy, 0.8, ends_type(("outflow", "outflow")), E.Sums(ny))
    return np.array_equal(out[1][:, 0], out[1][:, 1]) and np.array_equal(out[2][:, -1], out[2][:, -2])


def test_outflow_copies_what_the_neighbour_receives():
    assert outflow_copies_what_the_neighbour_receives(E.Ends)


# ---- 3. the linear profile between two value ends ------------------------------------------------------------

def linear_profile_errors(tau, ends_type=E.Ends, start="linear", n_sub=6000, nx=16, ny=6):
    """u = 0, no-flux walls, _VALUE 1.0 left and 0.0 right: (max |C - (1 - (x + 0.5)/nx)|, max relative error of the
    left end's net per row against D/nx, sum over rows of |net left + net right|) after n_sub substeps.
    start "linear": the equilibrium of the expected profile.  It is a fixed point of the scheme: at rest the
    equilibrium of a linear C streams into itself, and halfway anti-bounce-back places the value half a cell outside
    the end column, where the line has it; only the non-equilibrium part settles, by (1 - 1/tau) per substep.  The
    run then shows that 6000 substeps keep it and accumulates their rounding.  start "uniform": C = 0.5 everywhere;
    the slowest mode decays as exp(-D (pi/nx)^2) per substep, which reaches the last place within n_sub only for the
    larger D (tau 1.0: e^-38, tau 1.7: e^-92; tau 0.6 would need 23000 substeps)."""
    D = (tau - 0.5) / 3.0
    zero = np.zeros((ny, nx))
    want = (1.0 - (np.arange(nx) + 0.5) / nx)[None, :] * np.ones((ny, nx))
    g = S.equilibrium(want if start == "linear" else np.full((ny, nx), 0.5), zero, zero)
    g, sums, _ = E.event(g, zero, zero, tau, n_sub, ends_type(("value", "value"), (1.0, 0.0)), E.Sums(ny))
    err_c = np.max(np.abs(S.concentration(g) - want))
    err_q = np.max(np.abs(sums.last[0] - D / nx)) / (D / nx)
    imbalance = np.sum(np.abs(sums.last[0] + sums.last[1]))
    return err_c, err_q, imbalance


@pytest.mark.parametrize("tau,start", [(0.6, "linear"), (1.0, "linear"), (1.7, "linear"), (1.0, "uniform"),
                                       (1.7, "uniform")])
def test_the_linear_profile_is_exact(tau, start):
    err_c, err_q, imbalance = linear_profile_errors(tau, start=start)
    print(f"tau {tau} from {start}: profile err {err_c:.3e}, flux rel err {err_q:.3e}, |in + out| {imbalance:.3e}")
    assert err_c <= 1e-12 and err_q <= 1e-11 and imbalance <= 1e-13


# ---- 4. a blob leaves through the outflow end ----------------------------------------------------------------

_BLOB = {}


def blob_run(ends_type=E.Ends, n_sub=3000, nx=64, ny=4, tau=0.8):
    """Plug flow ux = 0.05, C = 1 on columns 20 .. 29, _VALUE 0.0 left and _OUTFLOW right, accumulate-only uptake
    for the walls' totals; and the periodic twin.  Computed once per ends type."""
    if ends_type not in _BLOB:
        ux, uy = np.full((ny, nx), 0.05), np.zeros((ny, nx))
        c0 = np.zeros((ny, nx))
        c0[:, 20:30] = 1.0
        g0 = S.equilibrium(c0, ux, uy)
        ends = None if ends_type is None else ends_type(("value", "outflow"), (0.0, 0.0))
        g, sums, us = E.event(g0, ux, uy, tau, n_sub, ends, E.Sums(ny), U.Uptake(), U.Sums(nx))
        _BLOB[ends_type] = (S.concentration(g0), S.concentration(g), sums, us)
    return _BLOB[ends_type]


def blob_left(ends_type=E.Ends):
    C0, C1, sums, _ = blob_run(ends_type)
    return np.sum(C0), np.sum(C1), np.sum(sums.total[0]), np.sum(sums.total[1])


def test_a_blob_leaves_through_the_outflow_end():
    s0, s1, left, right = blob_left()
    print(f"sum(C) {s0:.6g} -> {s1:.6e}; totals left {left:.6e}, right {right:.6f}")
    assert abs(s0 - 40.0) <= 40 * 8 * EPS and abs(s1) < 1e-3 * 40.0
    assert abs(right + 40.0) <= 1e-2 and abs(left) <= 1e-2
    # the periodic twin still holds all of it: the pair is the point of the feature
    C0, C1, sums, us = blob_run(None)
    bound = U.budget_bound(C0.size, 3000, C0.shape[1], max(np.sum(np.abs(C0)), np.sum(np.abs(C1))))
    print(f"periodic twin: sum(C) {np.sum(C1):.12f}, bound {bound:.3e}")
    assert abs(np.sum(C1) - 40.0) <= bound and sums.substeps == 0
    assert np.array_equal(us.total, np.zeros_like(us.total))


# ---- 5. the budget -------------------------------------------------------------------------------------------

def test_budget_of_the_outflow_run():
    C0, C1, sums, us = blob_run()
    ny, nx = C0.shape
    got = np.sum(C1) - np.sum(C0)
    want = np.sum(sums.total[0] + sums.total[1]) + np.sum(us.total[0] + us.total[1])
    bound = E.budget_bound(C0.size, 3000, nx, ny, max(np.sum(np.abs(C0)), np.sum(np.abs(C1))))
    print(f"d sum(C) {got:.6e}, totals {want:.6e}, |diff| {abs(got - want):.3e}, bound {bound:.3e}")
    assert sums.substeps == us.substeps == 3000
    assert abs(got - want) <= bound
    assert abs(got - np.sum(sums.total[0])) > 1e6 * bound  # the right end left out misses


@pytest.mark.parametrize("kind", [("value", "outflow"), ("outflow", "value"), ("outflow", "outflow"), ("value", "value"),
                                  ("noflux", "outflow")])
@pytest.mark.parametrize("nx,ny", [(20, 18), (37, 23), (16, 300)])
def test_budget_over_21_substeps_with_reactive_walls(nx, ny, kind):
    rng = np.random.default_rng(nx * 31 + ny)
    g, ux, uy = random_state(rng, nx, ny)
    up = U.Uptake((rng.uniform(0.0, 2.0, nx), rng.uniform(0.0, 2.0, nx)))
    ends = E.Ends(kind, (0.3, 0.6), (rng.uniform(0.0, 1.0, ny) if kind[0] == "value" else None, None))
    C0 = S.concentration(g)
    g1, sums, us = E.event(g, ux, uy, 0.8, 21, ends, E.Sums(ny), up, U.Sums(nx))
    C1 = S.concentration(g1)
    got = np.sum(C1) - np.sum(C0)
    want = np.sum(sums.total[0] + sums.total[1]) + np.sum(us.total[0] + us.total[1])
    bound = E.budget_bound(nx * ny, 21, nx, ny, max(np.sum(np.abs(C0)), np.sum(np.abs(C1))))
    print(f"{nx} x {ny} {kind}: d sum(C) {got:.6e}, totals {want:.6e}, |diff| {abs(got - want):.3e}, bound {bound:.3e}")
    assert sums.substeps == us.substeps == 21
    assert abs(got - want) <= bound
    # either family of accumulators left out misses by orders of magnitude
    assert abs(got - np.sum(us.total)) > 1e6 * bound and abs(got - np.sum(sums.total)) > 1e6 * bound


# ---- 6. no flux ----------------------------------------------------------------------------------------------

def test_no_flux_ends_between_no_flux_walls_conserve():
    rng = np.random.default_rng(94)
    nx, ny = 16, 6
    g, ux, uy = random_state(rng, nx, ny)
    C0 = S.concentration(g)
    g1, sums, _ = E.event(g, ux, uy, 0.8, 200, E.Ends(("noflux", "noflux")), E.Sums(ny))
    C1 = S.concentration(g1)
    bound = E.budget_bound(nx * ny, 200, nx, ny, max(np.sum(np.abs(C0)), np.sum(np.abs(C1))))
    print(f"d sum(C) {np.sum(C1) - np.sum(C0):.3e}, bound {bound:.3e}")
    assert abs(np.sum(C1) - np.sum(C0)) <= bound
    assert np.array_equal(sums.total, np.zeros((2, ny))) and np.array_equal(sums.last, np.zeros((2, ny)))
    assert sums.substeps == 200
    # it is not the periodic run
    assert not np.array_equal(g1, S.event(g, ux, uy, 0.8, 200))


# ---- 7. the seeded mistakes are told apart -------------------------------------------------------------------

def test_the_seeded_mistakes_are_told_apart():
    # an outflow end that takes the neighbour's population
    assert not outflow_copies_what_the_neighbour_receives(NeighbourOutflow)
    # a value end with the sign of q flipped misses the linear profile and its flux
    err_c, err_q, imbalance = linear_profile_errors(1.0, FlippedValue, n_sub=600)
    print(f"flipped value: profile err {err_c:.3e}, flux rel err {err_q:.3e}")
    assert not (err_c <= 1e-12 and err_q <= 1e-11)
    # (the blob does not tell it apart: at the value 0.0 the flipped end is a no-flux end, upstream of the blob)


# ---- 8. substeps count `stride` per event --------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 5, 7])
def test_substeps_count_stride_per_event(stride):
    rng = np.random.default_rng(95)
    nx, ny = 6, 4
    g, ux, uy = random_state(rng, nx, ny)
    ends = E.Ends(("value", "outflow"), (0.4, 0.0))
    sums, events = E.Sums(ny), 0
    for n, due in S.pieces([9, 11], 2, scalar=(2, stride)):
        if due["scalar"]:
            g, sums, _ = E.event(g, ux, uy, 0.8, stride, ends, sums)
            events += 1
            assert sums.substeps == stride * events
    assert events == 20 // stride
