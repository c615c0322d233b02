"""numpy restatement of the passive scalar's update rule with a source (include/iblb.h iblb_set_scalar_source), built
on scalar_ref.py: arrays shaped like Lattice.scalar_populations / Lattice.fields output.

Every arithmetic step is one numpy operation, in the order the header states, and no term is skipped for a missing
array or a zero decay: the results are meant to be compared with `==`.
"""
import numpy as np

import scalar_ref as S


class Source:
    """What Lattice.set_scalar_source takes: source (ny, nx) or None, decay, wall_flux / wall_value pairs of [nx] or
    None."""

    def __init__(self, source=None, decay=0.0, wall_flux=(None, None), wall_value=(None, None)):
        self.source, self.decay = source, float(decay)
        self.wall_flux, self.wall_value = tuple(wall_flux), tuple(wall_value)

    def kwargs(self):
        return dict(source=self.source, decay=self.decay, wall_flux=self.wall_flux, wall_value=self.wall_value)

    def present(self):
        bits = 1 | (2 if self.source is not None else 0)
        for k in range(2):
            bits |= (4 << k) if self.wall_flux[k] is not None else 0
            bits |= (16 << k) if self.wall_value[k] is not None else 0
        return bits


def rate(C, src):
    """r = s - decay*C, (ny, nx)."""
    s = np.zeros_like(C) if src.source is None else np.asarray(src.source, dtype=np.float64).reshape(C.shape)
    m = src.decay * C
    return s - m


def _wall(a, nx, default):
    return np.full(nx, float(default)) if a is None else np.asarray(a, dtype=np.float64).reshape(nx)


def substep(g, ux, uy, tau, src, walls=S.NO_FLUX_WALLS):
    """One substep of the populations g (5, ny, nx) at the velocity (ux, uy) with the source src."""
    g = np.asarray(g, dtype=np.float64)
    ux, uy = np.asarray(ux, dtype=np.float64), np.asarray(uy, dtype=np.float64)
    omega = 1.0 / float(tau)
    nx = g.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        C = S.concentration(g)
        r = rate(C, src)
        p = []
        for i, a in enumerate(S._directions(ux, uy)):
            geq = (S.W[i] * C) * (1.0 + 3.0 * a)
            p.append((g[i] - omega * (g[i] - geq)) + S.W[i] * r)
        out = np.empty_like(g)
        out[0] = p[0]
        out[1] = np.roll(p[1], 1, axis=1)
        out[2] = np.roll(p[2], -1, axis=1)
        out[3][1:] = p[3][:-1]
        out[4][:-1] = p[4][1:]
        for k, (row, plane, q) in enumerate(((0, 3, p[4][0]), (-1, 4, p[3][-1]))):
            kind, value = walls[k]
            if kind == S.VALUE:
                out[plane][row] = (2.0 * S.W1) * _wall(src.wall_value[k], nx, value) - q
            else:
                out[plane][row] = q + _wall(src.wall_flux[k], nx, 0.0)
    return out


def event(g, ux, uy, tau, stride, src, walls=S.NO_FLUX_WALLS):
    """One event: `stride` substeps with the velocity held fixed; src None: the rule without a source."""
    if src is None:
        return S.event(g, ux, uy, tau, stride, walls)
    for _ in range(stride):
        g = substep(g, ux, uy, tau, src, walls)
    return g


def wall_flux(g, src, walls=S.NO_FLUX_WALLS):
    """(bottom, top) as iblb_get_scalar_wall_flux returns them for the stored populations g with the source src."""
    nx = g.shape[2]
    out = []
    for k, stored in enumerate((g[3][0], g[4][-1])):
        kind, value = walls[k]
        if kind == S.VALUE:
            out.append(2.0 * stored - (2.0 * S.W1) * _wall(src.wall_value[k], nx, value))
        else:
            out.append(_wall(src.wall_flux[k], nx, 0.0))
    return tuple(out)
