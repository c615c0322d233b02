"""TEST INFRASTRUCTURE: the point-schedule scenarios of tests/test_point_schedule_cases.py (CPU) and
tests/test_gpu_point_schedules.py (GPU), defined once.  Plain numpy, no GPU.

A scenario is a list of actions on one context, as the caller of include/iblb.h would issue them, and a
pure function points_at(g) that says, by the header's contract alone, which (s, u_s, epsilon) iteration
g uses.  g counts the iterations of the scenario from its start and runs on across a state reset (the
library's own count, iblb_get_step, restarts there: Scenario.resets) and across a checkpoint restart.

Actions (tuples):
  ("schedule", s, u_s, eps)   iblb_set_lagrangian_steps, arrays (n, 2 Ns) / (n, Ns); Ns may be 0
  ("points", s, u_s, eps)     iblb_set_lagrangian
  ("state",)                  iblb_set_state(RHO, U)
  ("step", n)                 iblb_step(n)
  ("check", name)             compare with the oracle here (the end of a scenario is always compared)
  ("save",)                   iblb_save_checkpoint
  ("load",)                   iblb_load_checkpoint into a fresh context (first action of a restart)

The contract (include/iblb.h, iblb_set_lagrangian_steps): iteration t0 + i uses entry i, t0 the step count
at the call, however iblb_step is cut; after the last entry the points stay the last entry's; a new
schedule, static points or a schedule of no points end the old one; iblb_set_state keeps a schedule and
re-bases it (iteration i of the new state uses entry i); a checkpoint holds the points in use, static
after the load.
"""
import os

import numpy as np

from test_gpu_bulk import _schedule, _swaying

NX, NY, SEED = 256, 96, 5
BODY = (1e-6, 0.0)
MAX_POINTS = 120
K = int(os.environ.get("IBLB_SWEEP_DEPTH", "7"))
# The flux column.  The flux bound is relative to the oracle's cumulative flux, which presumes that the sum
# is not a cancelled remainder of its terms.  At the default column (XDIM - 5) it is one: with this state
# the sum passes through zero at iteration 17 = 2K + 3, where scenarios C and E are compared (2.4e-7 against
# terms of 2e-5: any rounding of the terms counts 80-fold).  At column 100 the sum stays above its largest
# term at every compared iteration of every scenario (test_point_schedule_cases.py asserts it, from the
# oracle alone).  Like XDIM - 5 the column lies outside every band patch and trapezoid (filaments at 43,
# 64, 128, 192, 213, +-15 columns), so the flux comes from the cycle's deep sweep as it does by default.
FLUX_COLUMN = 100

P3 = _swaying(NX, n_fil=3, pts=40)  # 120 points, x near 43, 128, 213
P2 = _swaying(NX, n_fil=2, pts=40)  # 80 points, x near 64, 192
NONE = (np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))

# the GPU test's bounds against the oracle (tests/test_gpu_bulk.py::test_moving_points_band_cycle_matches_oracle):
# rho, ux, uy each relative to its maximum
FIELD_TOL = {"f64": 1e-10, "f32": 1e-4}
FORCE_TOL = {"f64": 1e-9, "f32": 1e-3}
FS_TOL = {"f64": 1e-5, "f32": 1e-2}
FLUX_TOL = {"f64": 1e-9, "f32": 1e-4}


def state():
    from cuda_iblb_11_amd import workloads as W
    return W.perturbed_state(NX, NY, SEED)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (m if m > 0 else 1.0))


class Scenario:
    def __init__(self, name, actions, points_at, restarts=None, wrong=None):
        self.name = name
        self.actions = actions
        self.points_at = points_at      # g -> (s, u_s, eps)
        self.restarts = restarts or {}  # name -> actions of a fresh context, starting with ("load",)
        self.wrong = wrong or {}        # name -> a wrong mapping g -> points (the CPU power check)

    @property
    def steps(self):
        return sum(a[1] for a in self.actions if a[0] == "step")

    @property
    def resets(self):
        """g at which iblb_set_state is called."""
        out, g = [], 0
        for a in self.actions:
            if a[0] == "step":
                g += a[1]
            elif a[0] == "state":
                out.append(g)
        return out

    @property
    def compared(self):
        """g at which the GPU test compares the scenario's own context with the oracle."""
        out, g = [], 0
        for a in self.actions:
            if a[0] == "step":
                g += a[1]
            elif a[0] == "check":
                out.append(g)
        return out + [g]

    @property
    def saved_at(self):
        g = 0
        for a in self.actions:
            if a[0] == "step":
                g += a[1]
            elif a[0] == "save":
                return g
        return None


def _late(points_at):
    """Every entry one iteration late."""
    return lambda g: points_at(max(g - 1, 0))


def _stack(entries):
    return tuple(np.stack([e[i] for e in entries]) for i in range(3))


def scenario_a():
    n = 1 + 3 * K + 5
    at = lambda g: P3(min(g, n - 1))
    acts = [("schedule",) + _schedule(P3, 0, n)] + [("step", m) for m in (1, K, 2, K + 3, K)]
    return Scenario("A", acts, at, wrong={"late": _late(at)})


def scenario_b():
    n = K + 3
    at = lambda g: P3(min(g, n - 1))
    acts = [("schedule",) + _schedule(P3, 0, n)] + [("step", m) for m in (1, 2 * K, K + 1)]
    return Scenario("B", acts, at, wrong={"late": _late(at), "wrapped": lambda g: P3(g % n)})


def scenario_c():
    t1, t2, t3, t4 = 1 + K, 2 * K + 3, 2 * K + 4, 3 * K + 4
    first = P3(0)

    def at(g):
        if g < t1:
            return P3(g)           # first schedule (its entries t1 .. 2K are never used)
        if g < t2:
            return P2(g)           # second schedule: entry i = P2(t1 + i), all K + 2 used
        if g < t4:
            return NONE            # the zero-point schedule
        return first               # static points

    empty = (np.zeros((1, 0), np.float32), np.zeros((1, 0), np.float32), np.zeros((1, 0), np.int32))
    acts = [("schedule",) + _schedule(P3, 0, 2 * K + 1), ("step", t1), ("check", "first schedule"),
            ("schedule",) + _schedule(P2, t1, K + 2), ("step", K + 2), ("check", "second schedule"),
            ("schedule",) + empty, ("step", 1), ("check", "points gone"), ("step", K), ("check", "no points"),
            ("points",) + first, ("step", K + 1)]
    assert t3 == t2 + 1
    return Scenario("C", acts, at, wrong={"late": _late(at)})


D_POINT = 7  # the point of scenario D whose epsilon goes to 0 (1 in P3's pattern: 7 % 11 != 5)


def scenario_d():
    n = 1 + 3 * K
    s0, _, eps0 = P3(0)
    gone = 1 + K // 2 + 1  # inside the first band cycle (iterations 1 .. K)

    def at(g):
        g = min(g, n - 1)
        eps = eps0.copy()
        if g >= gone:
            eps[D_POINT] = 0
        return s0, P3(g)[1], eps

    assert eps0[D_POINT] == 1
    acts = [("schedule",) + _stack([at(g) for g in range(n)]), ("step", 1), ("step", 3 * K)]
    return Scenario("D", acts, at, wrong={"late": _late(at)})


def _line(x, n=40):
    k = np.arange(n)
    s = np.empty(2 * n, np.float32)
    s[0::2], s[1::2] = x, 2.0 + k
    us = np.zeros(2 * n, np.float32)
    us[0::2] = 2e-3 * k / n
    return s, us, np.ones(n, np.int32)


def scenario_e():
    line = _line(40.3)
    t0, reset = 1 + K, 1 + K + K + 2
    n = 3 * K

    def at(g):
        if g < t0:
            return line
        if g < reset:
            return P3(g - t0)  # entry i of the schedule is P3(i)
        return P3(min(g - reset, n - 1))  # re-based: iteration i of the new state uses entry i

    def old(g):  # before the fix: entry 0 for the first t0 iterations of the new state, then on
        return at(g) if g < reset else P3(min(max(g - reset - t0, 0), n - 1))

    acts = [("points",) + line, ("step", t0), ("schedule",) + _schedule(P3, 0, n), ("step", K + 2),
            ("check", "before the reset"), ("state",), ("step", 1 + 2 * K)]
    return Scenario("E", acts, at, wrong={"not re-based": old})


def scenario_f():
    n = 1 + 3 * K
    save = 1 + K + 2
    at = lambda g: P3(min(g, n - 1))
    held = lambda g: P3(min(g, save - 1))  # restart (ii): the saved points stay
    acts = [("schedule",) + _schedule(P3, 0, n), ("step", save), ("save",), ("step", n - save)]
    restarts = {"continued": [("load",), ("schedule",) + _schedule(P3, save, n - save), ("step", n - save)],
                "held": [("load",), ("step", K + 1)]}
    sc = Scenario("F", acts, at, restarts=restarts)
    sc.restart_points_at = {"continued": at, "held": held}
    return sc


def scenarios():
    return {s.name: s for s in (scenario_a(), scenario_b(), scenario_c(), scenario_d(), scenario_e(), scenario_f())}


# ---- the oracle under a mapping g -> points ------------------------------------------------------------
def snapshot(sim):
    return {"rho": sim.rho.copy(), "u": sim.u.copy(), "force": sim.force.copy(), "F_s": sim.F_s.copy(), "flux": sim.flux}


def oracle_run(O, mapping, g0, g1, sim=None, marks=()):
    """oracle.Simulation stepped one iteration at a time over g0 .. g1-1 with mapping(g)'s points (a fresh
    one from the scenarios' state where sim is None).  Returns (sim, {g: snapshot after g iterations})."""
    from cuda_iblb_11_amd import workloads as W
    if sim is None:
        rho, u = state()
        sim = O.Simulation(NX, NY, W.TAU, W.TAU2, rho=rho, u=u, body_force=BODY, flux_column=FLUX_COLUMN)
    out = {}
    for g in range(g0, g1):
        sim.set_lagrangian(*mapping(g))
        sim.step(1)
        if g + 1 in marks:
            out[g + 1] = snapshot(sim)
    return sim, out


def reference(O, sc, mapping=None, every=False):
    """Snapshots of the oracle under the scenario's points_at (or another mapping) after every g at which a
    step call of the scenario ends (every: after every iteration); a fresh Simulation at every reset."""
    mapping = mapping or sc.points_at
    ends, g = set(), 0
    for a in sc.actions:
        if a[0] == "step":
            g += a[1]
            ends.add(g)
    if every:
        ends = set(range(1, sc.steps + 1))
    out, sim, g0 = {}, None, 0
    for stop in sc.resets + [sc.steps]:
        sim, got = oracle_run(O, mapping, g0, stop, sim=sim, marks=ends)
        out.update(got)
        sim, g0 = None, stop
    return out
