"""tests/tracer_ref.py (the numpy restatement the GPU tests compare with) against hand-computed cases
of the definitions in include/iblb.h: iblb_sample_points' bilinear sample and the tracer update rule."""
import numpy as np

import tracer_ref as T

NX, NY = 6, 5


def ramp():
    """field[y, x] = 100 y + x: every cell has its own value, exact in double"""
    return 100.0 * np.arange(NY)[:, None] + np.arange(NX)[None, :]


def one(field, x, y):
    return float(T.sample(field, np.array([x]), np.array([y]))[0])


def test_a_cell_centre_returns_that_cell():
    f = ramp()
    for x in range(NX):
        for y in range(NY):
            assert one(f, float(x), float(y)) == f[y, x]
    # and a non-finite neighbour with weight 0 is not hidden: 0 * inf is NaN, as on the device
    g = f.copy()
    g[2, 3] = np.inf
    assert one(g, 3.0, 2.0) == np.inf and np.isnan(one(g, 2.0, 2.0))


def test_weights_inside_a_cell():
    f = ramp()
    # a = 0.25, b = 0.5 between cells (1, 2), (2, 2), (1, 3), (2, 3): 201, 202, 301, 302
    assert one(f, 1.25, 2.5) == 0.5 * (0.75 * 201 + 0.25 * 202) + 0.5 * (0.75 * 301 + 0.25 * 302) == 251.25


def test_the_last_column_mixes_with_column_zero():
    f = ramp()
    # x in [XDIM-1, XDIM): columns 5 and 0 of row 1 (105, 100), a = 0.25
    assert one(f, NX - 1 + 0.25, 1.0) == 0.75 * 105 + 0.25 * 100 == 103.75
    i0, i1, j0, j1, a, b = T.cells(np.array([np.nextafter(float(NX), 0.0)]), np.array([0.0]), NX, NY)
    assert (i0[0], i1[0]) == (NX - 1, 0) and 0.0 < a[0] < 1.0


def test_the_top_row():
    f = ramp()
    i0, i1, j0, j1, a, b = T.cells(np.array([2.0]), np.array([NY - 1.0]), NX, NY)
    assert (j0[0], j1[0], b[0]) == (NY - 2, NY - 1, 1.0)
    assert one(f, 2.0, NY - 1.0) == f[NY - 1, 2]
    assert one(f, 2.5, NY - 1.0) == 0.5 * f[NY - 1, 2] + 0.5 * f[NY - 1, 3]
    assert one(f, 2.0, NY - 1.5) == 0.5 * f[NY - 2, 2] + 0.5 * f[NY - 1, 2]


def uniform(ux, uy):
    return np.full((NY, NX), ux), np.full((NY, NX), uy)


def test_plain_step_and_stride():
    ux, uy = uniform(0.25, -0.125)
    x, y, laps = T.advect(ux, uy, np.array([1.0]), np.array([2.0]), np.array([0], dtype=np.int32), 1)
    assert (x[0], y[0], laps[0]) == (1.25, 1.875, 0)
    x, y, laps = T.advect(ux, uy, np.array([1.0]), np.array([2.0]), np.array([0], dtype=np.int32), 4)
    assert (x[0], y[0], laps[0]) == (2.0, 1.5, 0)


def test_a_wrap_each_way_changes_laps():
    ux, uy = uniform(0.5, 0.0)
    x, y, laps = T.advect(ux, uy, np.array([NX - 0.25]), np.array([1.0]), np.array([3], dtype=np.int32), 1)
    assert (x[0], y[0], laps[0]) == (0.25, 1.0, 4)
    ux, uy = uniform(-0.5, 0.0)
    x, y, laps = T.advect(ux, uy, np.array([0.25]), np.array([1.0]), np.array([3], dtype=np.int32), 1)
    assert (x[0], y[0], laps[0]) == (NX - 0.25, 1.0, 2)
    # a tiny step below zero rounds to XDIM itself: still outside [0, XDIM), so x and laps stay
    ux, uy = uniform(-1e-20, 0.0)
    x, y, laps = T.advect(ux, uy, np.array([0.0]), np.array([1.0]), np.array([0], dtype=np.int32), 1)
    assert (x[0], laps[0]) == (0.0, 0)
    # more than one lattice length in one update: x and laps stay, y moves
    ux, uy = uniform(2.0 * NX + 1, 0.5)
    x, y, laps = T.advect(ux, uy, np.array([1.0]), np.array([1.0]), np.array([0], dtype=np.int32), 1)
    assert (x[0], y[0], laps[0]) == (1.0, 1.5, 0)


def test_the_clamp_at_both_walls():
    ux, uy = uniform(0.0, -0.5)
    x, y, laps = T.advect(ux, uy, np.array([1.0]), np.array([0.25]), np.array([0], dtype=np.int32), 1)
    assert (x[0], y[0]) == (1.0, 0.0)
    ux, uy = uniform(0.0, 0.5)
    x, y, laps = T.advect(ux, uy, np.array([1.0]), np.array([NY - 1.25]), np.array([0], dtype=np.int32), 1)
    assert (x[0], y[0]) == (1.0, NY - 1.0)
    # a tracer on the top row is sampled there (b = 1) and stays in range
    x, y, laps = T.advect(ux, uy, np.array([1.0]), np.array([NY - 1.0]), np.array([0], dtype=np.int32), 1)
    assert y[0] == NY - 1.0


def test_a_non_finite_velocity_leaves_the_tracer_in_place():
    for bad in (np.nan, np.inf):
        ux, uy = uniform(0.25, 0.25)
        ux[2, 3] = bad
        x0, y0 = np.array([2.5, 0.5]), np.array([1.5, 0.5])  # the first tracer's cells include (3, 2)
        x, y, laps = T.advect(ux, uy, x0, y0, np.array([7, 7], dtype=np.int32), 1)
        assert (x[0], y[0], laps[0]) == (2.5, 1.5, 7)
        assert (x[1], y[1], laps[1]) == (0.75, 0.75, 7)
        x, y, laps = T.advect(uy, ux, x0, y0, np.array([7, 7], dtype=np.int32), 1)  # uy non-finite
        assert (x[0], y[0], laps[0]) == (2.5, 1.5, 7)


def test_special_points_are_valid_positions():
    for nx, ny in ((20, 18), (37, 23)):
        x, y = T.special_points(nx, ny)
        assert np.all((x >= 0) & (x < nx) & (y >= 0) & (y <= ny - 1))
        i0, i1, j0, j1, a, b = T.cells(x, y, nx, ny)
        assert np.any(i1 == 0) and np.any(b == 1.0) and np.any((a == 0) & (b == 0))
