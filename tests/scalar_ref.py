"""numpy restatement of the passive scalar's update rule (include/iblb.h iblb_set_scalar) on arrays shaped like
Lattice.fields / Lattice.scalar_populations output (populations (5, ny, nx), fields (ny, nx)), and of the plan
iblb_step cuts its calls into for any number of observers' event sets.

Every arithmetic step is one numpy operation (numpy's elementwise kernels round once per operation and do not
contract a multiply and an add), in the order the header states: the results are meant to be compared with `==`.
"""
import numpy as np

W0 = 1.0 / 3.0
W1 = 1.0 / 6.0
W = (W0, W1, W1, W1, W1)
NOFLUX = 0
VALUE = 1
NO_FLUX_WALLS = ((NOFLUX, 0.0), (NOFLUX, 0.0))


def concentration(g):
    """C = (((g0 + g1) + g2) + g3) + g4."""
    return (((g[0] + g[1]) + g[2]) + g[3]) + g[4]


def _directions(ux, uy):
    return (np.zeros_like(ux), ux, -ux, uy, -uy)


def equilibrium(C, ux, uy):
    """geq_i = (w_i*C) * (1.0 + 3.0*a_i), a = (0, ux, -ux, uy, -uy): (5, ny, nx)."""
    C, ux, uy = (np.asarray(v, dtype=np.float64) for v in (C, ux, uy))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(W[i] * C) * (1.0 + 3.0 * a) for i, a in enumerate(_directions(ux, uy))])


def substep(g, ux, uy, tau, walls=NO_FLUX_WALLS):
    """One substep of the populations g (5, ny, nx) at the velocity (ux, uy), each (ny, nx).  walls:
    ((kind, value) below row 0, (kind, value) above row ny - 1)."""
    g = np.asarray(g, dtype=np.float64)
    ux, uy = np.asarray(ux, dtype=np.float64), np.asarray(uy, dtype=np.float64)
    omega = 1.0 / float(tau)
    with np.errstate(invalid="ignore", over="ignore"):
        C = concentration(g)
        p = []
        for i, a in enumerate(_directions(ux, uy)):
            geq = (W[i] * C) * (1.0 + 3.0 * a)
            p.append(g[i] - omega * (g[i] - geq))
        out = np.empty_like(g)
        out[0] = p[0]
        out[1] = np.roll(p[1], 1, axis=1)    # g1'(x, y) = p1(x - 1, y)
        out[2] = np.roll(p[2], -1, axis=1)   # g2'(x, y) = p2(x + 1, y)
        out[3][1:] = p[3][:-1]               # g3'(x, y) = p3(x, y - 1)
        out[4][:-1] = p[4][1:]               # g4'(x, y) = p4(x, y + 1)
        (k0, v0), (k1, v1) = walls
        out[3][0] = (2.0 * W1) * float(v0) - p[4][0] if k0 == VALUE else p[4][0]
        out[4][-1] = (2.0 * W1) * float(v1) - p[3][-1] if k1 == VALUE else p[3][-1]
    return out


def event(g, ux, uy, tau, stride, walls=NO_FLUX_WALLS):
    """One event: `stride` substeps with the velocity held fixed."""
    for _ in range(stride):
        g = substep(g, ux, uy, tau, walls)
    return g


def pieces(calls, t, **events):
    """The pieces iblb_step cuts `calls` (a list of step counts) into from the state at iteration t, for any number
    of event sets given by name: name=(t0, stride) (events after t0 + stride, t0 + 2 stride, ...; t0 <= t) or None.
    Returns [(iterations, {name: due?})]: a call is cut at the union of the sets, and with none a call is one piece."""
    nxt = {}
    for name, ev in events.items():
        if ev is None:
            continue
        t0, stride = ev
        if stride < 1 or t0 > t:
            raise ValueError("need stride >= 1 and t0 <= t")
        nxt[name] = t0 + stride * ((t - t0) // stride + 1)
    out = []
    for n in calls:
        while n > 0:
            p = min([n] + [e - t for e in nxt.values()])
            t, n = t + p, n - p
            due = {name: name in nxt and nxt[name] == t for name in events}
            out.append((p, due))
            for name in nxt:
                if due[name]:
                    nxt[name] += events[name][1]
    return out
