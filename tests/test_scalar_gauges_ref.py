"""tests/scalar_gauges_ref.py, the numpy restatement of the scalar's transport gauges, pinned on the CPU: the change of
sum(C) over a box equals the gauges' nets on its sides plus the walls', the ends' and the source's share, at every size
down to one column; plug flow of a uniform C reads C u; the steady profile between two value walls reads D / ny at
every level; a station at the last column reads nothing under open ends; one column feeds both entries of its station;
and the gauges never change what the rule in force returns.

The budgets on narrow lattices (1, 2, 3 columns) are covered here only; the device runs 1 x 2, 2 x 3 and 5 x 257
against the twin in tests/test_gpu_scalar_matrix.py."""
import numpy as np
import pytest

import scalar_ref as S
import scalar_source_ref as Q
import scalar_uptake_ref as U
import scalar_ends_ref as E
import scalar_gauges_ref as G

TAU = 0.8
N_SUB = 40
MODES = ["periodic", "open ends", "uptake", "a source, uptake and open ends"]
# size: (stations, levels, the boxes as ((X0, X1), (Y0, Y1)); None: the box reaches the lattice's edge on that side)
BOXES = {
    (1, 5): ((0,), (0, 1, 3), [((None, None), (1, 3)), ((None, None), (None, 1)), ((None, None), (None, None))]),
    (2, 2): ((0, 1), (0,), [((0, 1), (0, None)), ((0, 1), (None, None))]),
    (3, 7): ((0, 1, 2), (1, 4, 5), [((0, 2), (1, 4)), ((0, 2), (None, None)), ((1, 2), (5, None))]),
    (20, 18): ((7, 19), (5, 16), [((7, 19), (5, 16)), ((7, 19), (None, None))]),
}


def random_state(rng, nx, ny):
    g = rng.uniform(0.1, 0.9, (5, ny, nx))
    ux, uy = rng.uniform(-0.05, 0.05, (2, ny, nx))
    return g, ux, uy


def setting(mode, rng, nx, ny):
    """(ends, uptake, source) of one mode."""
    ends = E.Ends(("value", "outflow"), (0.7, 0.0)) if "ends" in mode else None
    up = U.Uptake((rng.uniform(0.0, 2.0, nx), rng.uniform(0.0, 2.0, nx))) if "uptake" in mode else None
    src = Q.Source(rng.uniform(-2e-3, 4e-3, (ny, nx)), 0.02, (rng.uniform(-3e-3, 3e-3, nx), None)) if "source" in mode else None
    return ends, up, src


_RUNS = {}


def run(nx, ny, mode):
    """N_SUB substeps of a random state, one at a time so that the source's rate can be summed; computed once."""
    if (nx, ny, mode) not in _RUNS:
        rng = np.random.default_rng(nx * 131 + ny)
        g0, ux, uy = random_state(rng, nx, ny)
        ends, up, src = setting(mode, rng, nx, ny)
        ga = G.Gauges(*BOXES[(nx, ny)][:2])
        g, sums = g0, G.Sums(ga, nx, ny)
        es, us = (None if ends is None else E.Sums(ny)), (None if up is None else U.Sums(nx))
        r_sum = np.zeros((ny, nx))
        for _ in range(N_SUB):
            if src is not None:
                r_sum = r_sum + Q.rate(S.concentration(g), src)
            g, sums, es, us = G.substep(g, ux, uy, TAU, ga, sums, ends, es, up, us, src)
        for a in (g0, g, r_sum):
            a.setflags(write=False)
        _RUNS[(nx, ny, mode)] = (ga, g0, g, sums, es, us, r_sum, ends is not None)
    return _RUNS[(nx, ny, mode)]


def budget(nx, ny, mode, cols, rows, leave_out_gauges=False):
    """(|d sum(C over the box) - everything that entered it|, the bound, d sum(C))."""
    ga, g0, g1, sums, es, us, r_sum, open_ends = run(nx, ny, mode)
    X0, X1 = cols
    if open_ends and X1 == nx - 1:
        X1 = None  # no link right of the last column: that side is the end
    xs = slice(0 if X0 is None else X0 + 1, nx if X1 is None else X1 + 1)
    ys = slice(0 if rows[0] is None else rows[0] + 1, ny if rows[1] is None else rows[1] + 1)
    C0, C1 = S.concentration(g0)[ys, xs], S.concentration(g1)[ys, xs]
    entered, n_st, n_lv = G.box_net(ga, sums, (X0, X1), rows, nx, ny)
    if leave_out_gauges:
        entered = 0.0
    if open_ends:  # (periodic: a box without stations spans the whole width, and what wraps cancels)
        if X0 is None:
            entered = entered + np.sum(es.total[0][ys])
        if X1 is None:
            entered = entered + np.sum(es.total[1][ys])
    if us is not None:
        if rows[0] is None:
            entered = entered + np.sum(us.total[0][xs])
        if rows[1] is None:
            entered = entered + np.sum(us.total[1][xs])
    entered = entered + np.sum(r_sum[ys, xs])
    got = np.sum(C1) - np.sum(C0)
    bound = G.budget_bound(C0.size, N_SUB, nx, ny, max(np.sum(np.abs(C0)), np.sum(np.abs(C1))), n_st, n_lv)
    return abs(got - entered), bound, got


# ---- 1. the budgets ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nx,ny", list(BOXES))
def test_box_and_strip_budgets_close(nx, ny, mode):
    ga, _, _, sums, es, us, _, _ = run(nx, ny, mode)
    assert sums.substeps == N_SUB and sums.right.shape == sums.left.shape == (len(ga.stations), ny)
    assert sums.up.shape == sums.down.shape == (len(ga.levels), nx)
    for cols, rows in BOXES[(nx, ny)][2]:
        miss, bound, got = budget(nx, ny, mode, cols, rows)
        print(f"{nx} x {ny} {mode}: columns {cols} rows {rows}: d sum(C) {got:.6e}, |diff| {miss:.3e}, bound {bound:.3e}")
        assert miss <= bound, (cols, rows)


def test_the_figures_of_20_x_18():
    """Periodic, tau 0.8, a random velocity field, 40 substeps: the box of the columns (7, 19] and the rows (5, 16] and
    the strip of full height close to 7.5e-13 of 8.02 and 1.3e-12 of 8.43 with this seed (1.7e-13 of 1.135 and 1.8e-13
    with the state the feature was proposed on), a fortieth of the bound; without the gauges' nets either budget
    misses by all of d sum(C), more than 1e3 bounds."""
    for cols, rows in BOXES[(20, 18)][2]:
        miss, bound, got = budget(20, 18, "periodic", cols, rows)
        missed, _, _ = budget(20, 18, "periodic", cols, rows, leave_out_gauges=True)
        print(f"columns {cols} rows {rows}: d sum(C) {got:.4f}, |diff| {miss:.2e}, bound {bound:.2e}, without {missed:.2e}")
        assert miss <= bound and missed > 1e3 * bound


# ---- 2. plug flow --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("u", [0.03, -0.011])
def test_plug_flow_of_a_uniform_c_reads_c_u(u):
    nx, ny, Cv = 8, 5, 0.7
    ux, uy = np.full((ny, nx), u), np.zeros((ny, nx))
    g = S.equilibrium(np.full((ny, nx), Cv), ux, uy)
    ga = G.Gauges((0, 3, 7), (1,))
    for n in range(5):
        g, sums, _, _ = G.substep(g, ux, uy, TAU, ga, G.Sums(ga, nx, ny))  # fresh sums: one substep's share
        net = sums.right - sums.left
        assert np.all(np.abs(net - Cv * u) <= 2 * np.spacing(abs(Cv * u))), (n, np.max(np.abs(net - Cv * u)))
        assert np.all(np.abs(sums.up - sums.down) <= 2 * np.spacing(Cv / 6.0))  # nothing net across a level


# ---- 3. the steady profile between two value walls -----------------------------------------------------------

def level_flux_errors(tau, n_sub=6000, nx=16, ny=6):
    """u = 0, _VALUE walls 1.0 below and 0.0 above, the equilibrium of C = 1 - (y + 0.5)/ny (a fixed point, as the
    ends' restatement test has it along x): (max |C - profile|, max relative error of every level's net per column and
    substep against D/ny) after n_sub substeps, the last of them gauged alone."""
    D = (tau - 0.5) / 3.0
    zero = np.zeros((ny, nx))
    want = (1.0 - (np.arange(ny) + 0.5) / ny)[:, None] * np.ones((ny, nx))
    walls = ((S.VALUE, 1.0), (S.VALUE, 0.0))
    ga = G.Gauges((), tuple(range(ny - 1)))
    g = S.event(S.equilibrium(want, zero, zero), zero, zero, tau, n_sub - 1, walls)
    g, sums, _, _ = G.substep(g, zero, zero, tau, ga, G.Sums(ga, nx, ny), walls=walls)
    net = sums.up - sums.down
    return np.max(np.abs(S.concentration(g) - want)), np.max(np.abs(net - D / ny)) / (D / ny)


@pytest.mark.parametrize("tau", [0.6, 1.0, 1.7])
def test_every_level_reads_the_steady_flux(tau):
    err_c, err_q = level_flux_errors(tau)
    print(f"tau {tau}: profile err {err_c:.3e}, flux rel err {err_q:.3e}")
    assert err_c <= 1e-12 and err_q <= 1e-11


# ---- 4. the edges --------------------------------------------------------------------------------------------

def test_a_station_at_the_last_column_reads_nothing_under_open_ends():
    rng = np.random.default_rng(7)
    nx, ny = 6, 4
    g, ux, uy = random_state(rng, nx, ny)
    ga = G.Gauges((0, nx - 1), (0,))
    ends = E.Ends(("value", "outflow"), (0.4, 0.0))
    g1, sums, es, _ = G.event(g, ux, uy, TAU, 5, ga, G.Sums(ga, nx, ny), ends, E.Sums(ny))
    assert np.array_equal(sums.right[1], np.zeros(ny)) and np.array_equal(sums.left[1], np.zeros(ny))
    assert np.all(sums.right[0] != 0.0) and np.all(sums.left[0] != 0.0) and sums.substeps == es.substeps == 5
    # periodic, the same station reads the wrap: p_1 of the last column and p_2 of column 0
    _, per, _, _ = G.substep(g, ux, uy, TAU, ga, G.Sums(ga, nx, ny))
    p = U.relaxed(g, ux, uy, TAU, None)
    assert np.array_equal(per.right[1], 0.0 + p[1][:, nx - 1]) and np.array_equal(per.left[1], 0.0 + p[2][:, 0])


def test_one_periodic_column_feeds_both_entries():
    rng = np.random.default_rng(8)
    nx, ny = 1, 5
    g, ux, uy = random_state(rng, nx, ny)
    ga = G.Gauges((0,), (2,))
    p = U.relaxed(g, ux, uy, TAU, None)
    g1, sums, _, _ = G.substep(g, ux, uy, TAU, ga, G.Sums(ga, nx, ny))
    assert np.array_equal(sums.right[0], 0.0 + p[1][:, 0]) and np.array_equal(sums.left[0], 0.0 + p[2][:, 0])
    assert np.array_equal(sums.up[0], 0.0 + p[3][2]) and np.array_equal(sums.down[0], 0.0 + p[4][3])
    p2 = U.relaxed(g1, ux, uy, TAU, None)
    _, sums2, _, _ = G.substep(g1, ux, uy, TAU, ga, sums)
    assert np.array_equal(sums2.right[0], sums.right[0] + p2[1][:, 0]) and sums2.substeps == 2
    assert np.array_equal(sums.right[0], 0.0 + p[1][:, 0])  # the earlier Sums is not changed in place


# ---- 5. the gauges change nothing ----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_the_gauges_never_alter_what_the_rule_returns(mode):
    rng = np.random.default_rng(9)
    nx, ny = 7, 5
    g, ux, uy = random_state(rng, nx, ny)
    ends, up, src = setting(mode, rng, nx, ny)
    walls = ((S.VALUE, 0.25), (S.NOFLUX, 0.0))
    if up is not None:
        up = U.Uptake((None, up.rate[1]))  # no rate at the value wall
    if src is not None:
        src = Q.Source(src.source, src.decay)
    ga = G.Gauges((0, 1, nx - 1), (0, 1, ny - 2))
    es = None if ends is None else E.Sums(ny)
    us = None if up is None else U.Sums(nx)
    got, sums, ges, gus = G.event(g, ux, uy, TAU, 3, ga, G.Sums(ga, nx, ny), ends, es, up, us, src, walls)
    want, wes, wus = E.event(g, ux, uy, TAU, 3, ends, es, up, us, src, walls)
    assert np.array_equal(got, want) and sums.substeps == 3
    if ends is not None:
        assert np.array_equal(ges.total, wes.total) and np.array_equal(ges.last, wes.last)
    if up is not None:
        assert np.array_equal(gus.total, wus.total) and np.array_equal(gus.last, wus.last)
    # and without gauges the event is the existing one, the gauges' sums kept
    kept = G.Sums(ga, nx, ny)
    again, same, _, _ = G.event(g, ux, uy, TAU, 3, None, kept, ends, es, up, us, src, walls)
    assert same is kept and np.array_equal(again, want)
