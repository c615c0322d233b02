"""numpy restatement of the passive scalar's transport gauges (include/iblb.h iblb_set_scalar_gauges), built on
scalar_ref.py, scalar_source_ref.py, scalar_uptake_ref.py and scalar_ends_ref.py, all unchanged: arrays shaped like
Lattice.scalar_populations / Lattice.scalar_gauges output.

The populations, the uptake's sums and the ends' sums are those of the rule in force, taken from the existing
restatements: the gauges change none of them.  The gauges' own totals add the relaxed populations p_i of that rule
(scalar_uptake_ref.relaxed) that cross the gauged links, one numpy operation per addition: they are meant to be
compared with `==`.
"""
import numpy as np

import scalar_ref as S
import scalar_source_ref as Q
import scalar_uptake_ref as U
import scalar_ends_ref as E


class Gauges:
    """What Lattice.set_scalar_gauges takes: stations (columns) and levels (rows), strictly ascending."""

    def __init__(self, stations=(), levels=()):
        self.stations = tuple(int(x) for x in stations)
        self.levels = tuple(int(y) for y in levels)

    def kwargs(self):
        return dict(stations=self.stations, levels=self.levels)

    def info(self, substeps):
        return {"stations": self.stations, "levels": self.levels, "substeps": substeps}


class Sums:
    """The totals as Lattice.scalar_gauges returns them: right, left (n_stations, ny), up, down (n_levels, nx), and
    substeps.  Never changed in place: substep returns a new one."""

    def __init__(self, gauges, nx, ny, right=None, left=None, up=None, down=None, substeps=0):
        ns, nl = len(gauges.stations), len(gauges.levels)
        self.right = np.zeros((ns, ny)) if right is None else right
        self.left = np.zeros((ns, ny)) if left is None else left
        self.up = np.zeros((nl, nx)) if up is None else up
        self.down = np.zeros((nl, nx)) if down is None else down
        self.substeps = substeps


def substep(g, ux, uy, tau, gauges, sums, ends=None, end_sums=None, up=None, up_sums=None, src=None,
            walls=S.NO_FLUX_WALLS):
    """One substep with the gauges `gauges`: (populations, Sums of the gauges, Sums of the ends or None as given, Sums
    of the uptake or None).  ends None: the scalar is periodic in x."""
    g = np.asarray(g, dtype=np.float64)
    ux, uy = np.asarray(ux, dtype=np.float64), np.asarray(uy, dtype=np.float64)
    ny, nx = g.shape[1:]
    with np.errstate(invalid="ignore", over="ignore"):
        p = U.relaxed(g, ux, uy, tau, src)
        if ends is not None:
            out, end_sums, up_sums = E.substep(g, ux, uy, tau, ends, end_sums, up, up_sums, src, walls)
        else:
            out, up_sums = U.event(g, ux, uy, tau, 1, up, up_sums, src, walls)
        right, left = np.empty_like(sums.right), np.empty_like(sums.left)
        for k, X in enumerate(gauges.stations):
            if ends is not None and X == nx - 1:  # no link right of the last column: 0.0 to both
                right[k] = sums.right[k] + np.zeros(ny)
                left[k] = sums.left[k] + np.zeros(ny)
            else:
                right[k] = sums.right[k] + p[1][:, X]
                left[k] = sums.left[k] + p[2][:, (X + 1) % nx]
        upw, down = np.empty_like(sums.up), np.empty_like(sums.down)
        for k, Y in enumerate(gauges.levels):
            upw[k] = sums.up[k] + p[3][Y]
            down[k] = sums.down[k] + p[4][Y + 1]
    return out, Sums(gauges, nx, ny, right, left, upw, down, sums.substeps + 1), end_sums, up_sums


def event(g, ux, uy, tau, stride, gauges, sums, ends=None, end_sums=None, up=None, up_sums=None, src=None,
          walls=S.NO_FLUX_WALLS):
    """One event: `stride` substeps with the velocity held fixed: (populations, Sums of the gauges, of the ends, of the
    uptake).  gauges None: the rule in force by the existing restatements, the gauges' sums kept."""
    if gauges is None:
        g, end_sums, up_sums = E.event(g, ux, uy, tau, stride, ends, end_sums, up, up_sums, src, walls)
        return g, sums, end_sums, up_sums
    for _ in range(stride):
        g, sums, end_sums, up_sums = substep(g, ux, uy, tau, gauges, sums, ends, end_sums, up, up_sums, src, walls)
    return g, sums, end_sums, up_sums


def box_net(gauges, sums, cols, rows, nx, ny):
    """What the gauges saw enter the box of the columns X0 + 1 .. X1 and the rows Y0 + 1 .. Y1, cols = (X0, X1) and
    rows = (Y0, Y1): each a gauged position, or None for a side that is no gauge (X0 None: the box starts at column 0,
    X1 None: it ends at column nx - 1; Y0 None: it starts at row 0, Y1 None: it ends at row ny - 1): that side's
    share, a wall's or an end's total or nothing, is the caller's to add.  Returns (the net, the number of stations
    summed, the number of levels summed)."""
    (X0, X1), (Y0, Y1) = cols, rows
    xs = slice(0 if X0 is None else X0 + 1, nx if X1 is None else X1 + 1)
    ys = slice(0 if Y0 is None else Y0 + 1, ny if Y1 is None else Y1 + 1)
    net, n_st, n_lv = 0.0, 0, 0
    for X, sign in ((X0, 1.0), (X1, -1.0)):
        if X is not None:
            k = gauges.stations.index(X)
            net = net + sign * np.sum((sums.right[k] - sums.left[k])[ys])
            n_st += 1
    for Y, sign in ((Y0, 1.0), (Y1, -1.0)):
        if Y is not None:
            k = gauges.levels.index(Y)
            net = net + sign * np.sum((sums.up[k] - sums.down[k])[xs])
            n_lv += 1
    return net, n_st, n_lv


def budget_bound(n_cells, n_sub, nx, ny, scale, n_stations, n_levels):
    """The bound on |d sum(C over a box) - (the gauges' nets + the walls' and ends' totals + the box's source)| over
    n_sub substeps: the form of scalar_ends_ref.budget_bound (the two sums over the n_cells cells of the box, about
    eight roundings per cell and substep, the walls' and the ends' accumulators' own sums) with one more term per gauge
    entry summed, n_stations * ny + n_levels * nx for the stations and levels on the box's sides: each a half unit in
    the last place of `scale`, the larger sum |C| over the box of the two ends of the run."""
    return (2 * n_cells + 8 * n_sub + 2 * nx + 2 * ny + n_stations * ny + n_levels * nx) * 2.0 ** -53 * scale
