"""numpy restatement of the passive scalar's update rule with open ends in x (include/iblb.h iblb_set_scalar_ends), built
on scalar_ref.py, scalar_source_ref.py and scalar_uptake_ref.py: arrays shaped like Lattice.scalar_populations /
Lattice.scalar_ends output.

Every arithmetic step is one numpy operation, in the order the header states, and no term is skipped: the populations,
totals and last are meant to be compared with `==`.  The relaxation and the two wall rows are those of the rule in
force, taken from the existing restatements unchanged; only the streaming along x is written out here, without the
wrap, so that every element of the five output planes has one writer (`count` counts them).
"""
import numpy as np

import scalar_ref as S
import scalar_source_ref as Q
import scalar_uptake_ref as U

NOFLUX, VALUE, OUTFLOW = 0, 1, 2
KINDS = {"noflux": NOFLUX, "value": VALUE, "outflow": OUTFLOW}


class Ends:
    """What Lattice.set_scalar_ends takes: kind, value and profile, pairs (left of column 0, right of column nx - 1)."""

    def __init__(self, kind=("value", "outflow"), value=(0.0, 0.0), profile=(None, None)):
        self.kind = tuple(KINDS[k] if isinstance(k, str) else int(k) for k in kind)
        self.value = tuple(float(v) for v in value)
        self.profile = tuple(profile)

    def kwargs(self):
        return dict(kind=self.kind, value=self.value, profile=self.profile)

    def present(self):
        return 1 | (2 if self.profile[0] is not None else 0) | (4 if self.profile[1] is not None else 0)

    def v(self, k, ny):
        """The value of every row at end k: profile[k], or value[k] where it is None."""
        if self.profile[k] is None:
            return np.full(ny, self.value[k])
        return np.asarray(self.profile[k], dtype=np.float64).reshape(ny)

    def received(self, k, p, ny):
        """(what the end column's inward direction receives, q) at end k from the relaxed populations p: [ny] each."""
        col, leaving, inward = ((0, 2, 1), (-1, 1, 2))[k]
        q = p[leaving][:, col]
        if self.kind[k] == VALUE:
            return (2.0 * S.W1) * self.v(k, ny) - q, q
        if self.kind[k] == OUTFLOW:
            return p[inward][:, col], q
        return q, q


class Sums:
    """The accumulators as Lattice.scalar_ends returns them: total and last, (2, ny) each ([0] left, [1] right), and
    substeps.  Never changed in place: substep returns a new one."""

    def __init__(self, ny, total=None, last=None, substeps=0):
        self.total = np.zeros((2, ny)) if total is None else total
        self.last = np.zeros((2, ny)) if last is None else last
        self.substeps = substeps


def _rule_in_force(g, ux, uy, tau, up, up_sums, src, walls):
    """One substep of the periodic rule in force: (populations, the uptake's Sums or None)."""
    if up is not None:
        return U.substep(g, ux, uy, tau, up, up_sums, src, walls)
    if src is not None:
        return Q.substep(g, ux, uy, tau, src, walls), up_sums
    return S.substep(g, ux, uy, tau, walls), up_sums


def substep(g, ux, uy, tau, ends, sums, up=None, up_sums=None, src=None, walls=S.NO_FLUX_WALLS, count=None):
    """One substep with the ends `ends`: (populations, Sums of the ends, Sums of the uptake or None).  count: an int
    array shaped like g, or None; every store into the output adds one to the elements it writes."""
    g = np.asarray(g, dtype=np.float64)
    ux, uy = np.asarray(ux, dtype=np.float64), np.asarray(uy, dtype=np.float64)
    ny, nx = g.shape[1:]
    out = np.full_like(g, np.nan)

    def put(plane, rows, cols, a):
        out[plane][rows, cols] = a
        if count is not None:
            count[plane][rows, cols] += 1

    every = slice(None)
    with np.errstate(invalid="ignore", over="ignore"):
        periodic, up_sums = _rule_in_force(g, ux, uy, tau, up, up_sums, src, walls)
        p = U.relaxed(g, ux, uy, tau, src)
        put(0, every, every, p[0])
        put(1, every, slice(1, None), p[1][:, :-1])    # g1'(x, y) = p1(x - 1, y), x >= 1
        put(2, every, slice(None, -1), p[2][:, 1:])    # g2'(x, y) = p2(x + 1, y), x <= nx - 2
        put(3, slice(1, None), every, p[3][:-1])       # g3'(x, y) = p3(x, y - 1)
        put(4, slice(None, -1), every, p[4][1:])       # g4'(x, y) = p4(x, y + 1)
        put(3, slice(0, 1), every, periodic[3][0:1])   # the walls: the rule in force, whole rows, corners included
        put(4, slice(ny - 1, ny), every, periodic[4][ny - 1:ny])
        total, last = np.empty((2, ny)), np.empty((2, ny))
        for k, (plane, col) in enumerate(((1, slice(0, 1)), (2, slice(nx - 1, nx)))):
            new, q = ends.received(k, p, ny)
            net = new - q
            put(plane, every, col, new[:, None])
            total[k] = sums.total[k] + net
            last[k] = net
    return out, Sums(ny, total, last, sums.substeps + 1), up_sums


def event(g, ux, uy, tau, stride, ends, sums, up=None, up_sums=None, src=None, walls=S.NO_FLUX_WALLS):
    """One event: `stride` substeps with the velocity held fixed: (populations, Sums of the ends, Sums of the uptake).
    ends None: the periodic rule in force by the existing restatements, the ends' sums kept."""
    if ends is None:
        g, up_sums = U.event(g, ux, uy, tau, stride, up, up_sums, src, walls)
        return g, sums, up_sums
    for _ in range(stride):
        g, sums, up_sums = substep(g, ux, uy, tau, ends, sums, up, up_sums, src, walls)
    return g, sums, up_sums


def budget_bound(n_cells, n_sub, nx, ny, scale):
    """The bound on |d sum(C) - (the ends' totals + the walls' totals)| over n_sub substeps: the form of
    scalar_uptake_ref.budget_bound with 2 ny added for the ends' accumulators' own sums."""
    return (2 * n_cells + 8 * n_sub + 2 * nx + 2 * ny) * 2.0 ** -53 * scale
