"""TEST INFRASTRUCTURE: the on-device cilia (iblb_set_cilia) scenarios of tests/test_cilia_cases.py (CPU),
tests/test_gpu_cilia_paths.py (GPU) and tests/mock_rccl/run_cilia.py (RCCL slabs), defined once.  Plain
numpy, no GPU.

Two configurations (both on 192 rows, T = 1e5, p_step = T // c_num, the reference's own phase lag):

  WIDE  4 cilia 128 apart on 512 x 192: the cilia lie around x = 22 .. 448, away from the periodic seam, and the
        lattice is wide enough for the band planner to accept their trapezoids at depth 5 (f64 and f32).
  REF   the reference's defaults, 6 cilia 48 apart on 288 x 192: the outermost points sit at s_x = 0.6 and
        287.9 from iteration 0 (their 3 x 3 nodes cross the periodic seam), and a cilium base stands on the
        edge of two slabs (x = 144).

The reference's penalty IB is linearly unstable: the fluid of both configurations
exceeds |u| = 0.1 before iteration 40.  Every compared run stays inside HORIZON iterations counted from the
last iblb_set_state (WIDE 23, REF 15: what tests/test_gpu_fused.py already compares), and
tests/test_cilia_cases.py asserts max|u| <= 0.03 at the end of every case.

A case is a list of actions executed by both sides, the library and the oracle twin:

  ("step", n)             iblb_step(n) / n oracle iterations, one at a time, with Cilia.points(it)
  ("set_state", seed)     iblb_set_state(perturbed_state(seed)) / a fresh Simulation and a fresh Cilia, `it`
                          restarting at 0 (main.cu:348-359: the beat restarts with the state)
  ("cilia_off", points)   iblb_set_cilia(off) then iblb_set_lagrangian(points) / the twin's point source
                          becomes the static points

The twin (Twin) can be given one of three sequencing faults, for the CPU power check: `shift` (every `it` of
the kinematics off by that much), `fresh_at` (a fresh Cilia, zeroed history, at those iteration counts, the
hand-over between two calls), `keep_beat` (no restart of the kinematics at a state reset).
"""
import numpy as np

NY = 192
T_BEAT = 100000
BODY = (1e-6, 0.0)
SEED = 11
K = 5  # the depth the call lists are built from (IBLB_SWEEP_DEPTH=5 where band cycles are wanted)


class Config:
    def __init__(self, name, c_num, c_space, horizon):
        self.name, self.c_num, self.c_space, self.T = name, int(c_num), float(c_space), T_BEAT
        self.nx, self.ny = int(c_num * c_space), NY
        self.p_step = self.T // self.c_num
        self.max_points = 96 * self.c_num
        self.horizon = horizon

    @property
    def cilia(self):
        """The arguments of Lattice.set_cilia."""
        return self.c_num, self.c_space, self.T, self.p_step

    def state(self, seed=SEED):
        from cuda_iblb_11_amd import workloads as W
        return W.perturbed_state(self.nx, self.ny, seed)


WIDE = Config("WIDE", 4, 128.0, 23)
REF = Config("REF", 6, 48.0, 15)
CONFIGS = {"WIDE": WIDE, "REF": REF}

# the bounds against the oracle of tests/test_gpu_fused.py::test_cilia_band_cycle and
# ::test_reference_cilia_scenario: rho, ux, uy each relative to its maximum
FIELD_TOL = {"f64": 1e-9, "f32": 1e-4}


def rel(a, b):
    """max|a - b| / max|b|; inf where a is not finite (a blown-up twin differs by any measure)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        return float("inf")
    m = np.max(np.abs(b)) if b.size else 1.0
    return float(np.max(np.abs(a - b)) / (m if m > 0 else 1.0)) if a.size else 0.0


def fields_rel(rho, u, rho_ref, u_ref):
    n = rho_ref.size
    return {"rho": rel(rho, rho_ref), "rho-1": rel(rho - 1, rho_ref - 1), "ux": rel(u[:n], u_ref[:n]),
            "uy": rel(u[n:], u_ref[n:])}


def static_points(cfg, n=24):
    """The static points case 5 switches to: one 24-point filament between two cilia."""
    from cuda_iblb_11_amd import workloads as W
    return W.filament(3, n_points=n, x0=cfg.nx / 2 + 40.3, y0=20.0, dy=1.0, U0=2e-3, period=12, sway=1.5)


# ---- the cases (lone slab; K = 5) ------------------------------------------------------------------------
def steps(*calls):
    return [("step", n) for n in calls]


def case1(k=4):
    """Consecutive schedules with one-step remainders inside, a short call, a schedule again.  The call list
    (1, 2K + 3, K + 1, 2, K) is 4K + 7 iterations: 27 at depth 5, past WIDE's horizon of 23, and no list of
    that shape with four band cycles fits 23 iterations at depth 5 (1 + (3K + 2) + 1 + K = 24).  At depth 4
    it is exactly 23, so this one case is built from, and run at, depth 4."""
    return steps(1, 2 * k + 3, k + 1, 2, k)


CASE2_WIDE = steps(1 + K + 2) + [("set_state", SEED + 1)] + steps(1 + 2 * K, 3)
CASE2_REF = steps(4) + [("set_state", SEED + 1)] + steps(6, 3)
CASE3 = {"cycle": (1 + K, 2 * K + 2), "owed": (1 + K + 2, 2 * K + 2)}  # (before the save, after it)
CASE4_STEPS = 1 + 20
CASE6 = steps(1, K, K + 2)
GROUP_CALLS = (1, 5, 6)


def case5(cfg=WIDE):
    return steps(1 + K) + [("cilia_off", static_points(cfg))] + steps(K + 2)


def total(actions):
    """The longest run of iterations between two state resets, and the iterations in all."""
    longest = cur = n = 0
    for a in actions:
        if a[0] == "step":
            cur, n = cur + a[1], n + a[1]
        elif a[0] == "set_state":
            cur = 0
        longest = max(longest, cur)
    return longest, n


# ---- the oracle twin -------------------------------------------------------------------------------------
class Twin:
    """oracle.Simulation stepped one iteration at a time with oracle.Cilia.points(it)."""

    def __init__(self, O, cfg, seed=SEED, body=BODY, flux_column=None, shift=0, fresh_at=(), keep_beat=False):
        self.O, self.cfg, self.body, self.flux_column = O, cfg, body, flux_column
        self.shift, self.fresh_at, self.keep_beat = int(shift), set(fresh_at), bool(keep_beat)
        self.g = 0          # iterations of the whole case
        self.static = None  # the static points after ("cilia_off", points)
        self.cil = None
        self.set_state(seed)

    def _new_cilia(self):
        c = self.cfg
        return self.O.Cilia(c.c_num, c.c_space, c.T, c.p_step, c.nx)

    def set_state(self, seed):
        from cuda_iblb_11_amd import workloads as W
        c = self.cfg
        rho, u = c.state(seed)
        self.sim = self.O.Simulation(c.nx, c.ny, W.TAU, W.TAU2, rho=rho, u=u, body_force=self.body,
                                     flux_column=self.flux_column)
        if self.cil is None or not self.keep_beat:
            self.cil, self.it = self._new_cilia(), 0

    def cilia_off(self, points):
        self.static = tuple(np.array(p) for p in points)

    def step(self, n=1):
        for _ in range(n):
            if self.static is not None:
                self.sim.set_lagrangian(*self.static)
            else:
                if self.g in self.fresh_at:
                    self.cil = self._new_cilia()
                self.sim.set_lagrangian(*self.cil.points(self.it + self.shift))
            self.sim.step(1)
            self.it += 1
            self.g += 1

    def points(self):
        """(s, u_s, epsilon) in use by the last iteration."""
        return self.static if self.static is not None else (self.cil.s, self.cil.u_s, self.cil.epsilon)

    def snapshot(self):
        s, us, eps = self.points()
        return {"rho": self.sim.rho.copy(), "u": self.sim.u.copy(), "flux": self.sim.flux, "F_s": self.sim.F_s.copy(),
                "s": np.array(s), "u_s": np.array(us), "eps": np.array(eps), "g": self.g}


def run_twin(O, cfg, actions, **kw):
    """The twin through an action list; a snapshot after every ("step", n).  Returns (twin, [snapshot])."""
    tw = Twin(O, cfg, **kw)
    out = []
    for a in actions:
        if a[0] == "step":
            tw.step(a[1])
            out.append(tw.snapshot())
        elif a[0] == "set_state":
            tw.set_state(a[1])
        elif a[0] == "cilia_off":
            tw.cilia_off(a[1])
        else:
            raise ValueError(a[0])
    return tw, out


def run_lattice(lat, cfg, actions, after_step=None):
    """The same action list on a Lattice (or anything with its step / set_state / set_cilia /
    set_lagrangian): after_step(i, lat) runs after the i-th ("step", n)."""
    i = 0
    for a in actions:
        if a[0] == "step":
            lat.step(a[1])
            if after_step:
                after_step(i, lat)
            i += 1
        elif a[0] == "set_state":
            lat.set_state(*cfg.state(a[1]))
        elif a[0] == "cilia_off":
            lat.set_cilia(0, cfg.c_space, cfg.T, cfg.p_step)
            lat.set_lagrangian(*a[1])
        else:
            raise ValueError(a[0])


# ---- the band planner's input for a cycle (csrc/ctx_band.hip:plan_cycle) -----------------------------------
def cycle_points(O, cfg, t, k):
    """(x, y) of every point a band cycle of depth k starting at iteration t >= 1 may see: the points of
    iterations t - 1 .. t + k - 2."""
    cil = O.Cilia(cfg.c_num, cfg.c_space, cfg.T, cfg.p_step, cfg.nx)
    xy = []
    for it in range(t + k - 1):
        s = cil.points(it)[0]
        if it >= t - 1:
            xy.append(s.copy())
    return np.concatenate(xy)
