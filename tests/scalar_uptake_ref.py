"""numpy restatement of the passive scalar's update rule with an uptake (include/iblb.h iblb_set_scalar_uptake), built
on scalar_ref.py and scalar_source_ref.py: arrays shaped like Lattice.scalar_populations / Lattice.scalar_uptake
output.

Every arithmetic step is one numpy operation, in the order the header states, and no term is skipped for a missing
array: the populations, totals and last are meant to be compared with `==`.
"""
import numpy as np

import scalar_ref as S
import scalar_source_ref as Q


class Uptake:
    """What Lattice.set_scalar_uptake takes: rate, a pair of [nx] or None (below row 0, above the top row)."""

    def __init__(self, rate=(None, None)):
        self.rate = tuple(rate)

    def kwargs(self):
        return dict(rate=self.rate)

    def present(self):
        return 1 | (2 if self.rate[0] is not None else 0) | (4 if self.rate[1] is not None else 0)

    def coefficient(self, k, nx):
        """a_k[x] = 2.0 - 2.0/(1.0 + 3.0*rate[k][x]); 0.0 where rate[k] is None."""
        if self.rate[k] is None:
            return np.zeros(nx)
        r = np.asarray(self.rate[k], dtype=np.float64).reshape(nx)
        with np.errstate(over="ignore"):
            return 2.0 - 2.0 / (1.0 + 3.0 * r)


class Sums:
    """The accumulators as Lattice.scalar_uptake returns them: total and last, (2, nx) each ([0] bottom, [1] top),
    and substeps.  Never changed in place: substep returns a new one."""

    def __init__(self, nx, total=None, last=None, substeps=0):
        self.total = np.zeros((2, nx)) if total is None else total
        self.last = np.zeros((2, nx)) if last is None else last
        self.substeps = substeps


def relaxed(g, ux, uy, tau, src):
    """p_i of the rule in force: that of iblb_set_scalar (src None) or of iblb_set_scalar_source."""
    omega = 1.0 / float(tau)
    C = S.concentration(g)
    r = None if src is None else Q.rate(C, src)
    p = []
    for i, a in enumerate(S._directions(ux, uy)):
        geq = (S.W[i] * C) * (1.0 + 3.0 * a)
        pi = g[i] - omega * (g[i] - geq)
        p.append(pi if src is None else pi + S.W[i] * r)
    return p


def substep(g, ux, uy, tau, up, sums, src=None, walls=S.NO_FLUX_WALLS):
    """One substep with the uptake `up`: (populations, Sums)."""
    g = np.asarray(g, dtype=np.float64)
    ux, uy = np.asarray(ux, dtype=np.float64), np.asarray(uy, dtype=np.float64)
    nx = g.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        p = relaxed(g, ux, uy, tau, src)
        out = np.empty_like(g)
        out[0] = p[0]
        out[1] = np.roll(p[1], 1, axis=1)
        out[2] = np.roll(p[2], -1, axis=1)
        out[3][1:] = p[3][:-1]
        out[4][:-1] = p[4][1:]
        total, last = np.empty((2, nx)), np.empty((2, nx))
        for k, (row, plane, q) in enumerate(((0, 3, p[4][0]), (-1, 4, p[3][-1]))):
            kind, value = walls[k]
            if kind == S.VALUE:
                wv = np.full(nx, float(value)) if src is None else Q._wall(src.wall_value[k], nx, value)
                new = (2.0 * S.W1) * wv - q
                net = new - q
            else:
                e = np.zeros(nx) if src is None else Q._wall(src.wall_flux[k], nx, 0.0)
                l = up.coefficient(k, nx) * q
                new = (q - l) + e
                net = e - l
            out[plane][row] = new
            total[k] = sums.total[k] + net
            last[k] = net
    return out, Sums(nx, total, last, sums.substeps + 1)


def event(g, ux, uy, tau, stride, up, sums, src=None, walls=S.NO_FLUX_WALLS):
    """One event: `stride` substeps with the velocity held fixed; up None: the rule without an uptake, sums kept."""
    if up is None:
        return Q.event(g, ux, uy, tau, stride, src, walls), sums
    for _ in range(stride):
        g, sums = substep(g, ux, uy, tau, up, sums, src, walls)
    return g, sums


def budget_bound(n_cells, n_sub, nx, scale):
    """The bound on |d sum(C) - sum_x(total_0 + total_1)| over n_sub substeps: the two sums' worst case (2 N), about
    eight roundings per cell and substep spread over sum_i |g_i| = C, and the accumulators' own sums (2 nx), each a
    half unit in the last place of `scale`, the larger sum |C| of the two ends."""
    return (2 * n_cells + 8 * n_sub + 2 * nx) * 2.0 ** -53 * scale
