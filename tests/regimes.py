"""The collide's parameter regimes (relaxation pair x state amplitude x body force, with an IB point
speed tied to the amplitude), shared by the CPU tests (tests/test_regimes.py) and the GPU tests
(tests/test_gpu_regimes.py).  Test infrastructure (numpy only).

Every other parity test runs the collide at one point: reference_taus() = (2.8068, 0.5361), a state
of amplitude 1e-3, a body force ~1e-6, IB point speeds ~1e-3.  There the nonlinear and the forcing
terms of the collide sit below the float32 rounding of the linear ones, and the folded constants
hs = (1 - w+)/2, hd = (1 - w-)/2 have one sign pattern.  The relaxation pairs here give w+ < 1 < w-
(Re1), w- < 1 < w+ (swapped, Re100), both below 1 (Re10), w+ = w- (BGK, low: a forcing constant taken
from the wrong relaxation time is invisible there and only there), omp = 1 - w+ exactly 0 (magic) and
both close to 2 (low); amplitude 3e-2 and the body force (1e-4, -5e-5) lift the quadratic and the
forcing terms two to four decades above float32 rounding.

Bounds.  f64: the suite's own (TIGHT = 1e-9 without IB; with IB fields 1e-10, force 1e-9, F_s 1e-5,
flux 1e-9), always on rho - 1.  f32 without IB: f32_bound = FACTOR x floor, floor = the worst of
rho - 1, u_x, u_y of the op-for-op CPU emulation of the f32 collide (tests/f32_gpu_model.py) against the
oracle for the same case, shape and iteration count; FACTOR covers what the emulation does not model
(v_rcp_f32 + one Newton step against an exact quotient, fma results on float32 ties).
FACTOR = 3, from GPU errors measured at 0.85 ... 1.154 x the floor over the 28 cases (the figures stand
at its definition below).  f32 with IB: f32_ib_bound = FACTOR_IB x ib_floor per quantity (rho - 1, u_x, u_y,
the dense force, F_s), ib_floor = the op-for-op CPU emulation of the IB iteration in the kernels' arithmetic
(f32_gpu_model.F32GpuIBChannel) against the oracle for the same case and configuration; the flux within
3 x the u_x bound x flux_scale, as without IB.  FACTOR_IB = 3 from GPU errors at 0.80 ... 1.5 x the floor (the
figures stand at its definition).  The earlier bounds (IB_TOL: 1e-4 on rho - 1, u_x, u_y, force 1e-3,
F_s 1e-2, flux 1e-4) stay asserted; f32_ib_bound is 20 (fields) to 2e4 (F_s) times below them.  Two f32 runs of the same
case on different IB paths differ at most by the arrival order of the spread atomics: ib_order_envelope.
"""
from __future__ import annotations

import functools
import itertools
from collections import namedtuple

import numpy as np

from cuda_iblb_11_amd import workloads as W
from cuda_iblb_11_amd.lattice import reference_taus

TOL32, TIGHT = 1e-4, 1e-9

# FACTOR = 2 x the largest GPU error / emulation floor over FULL, rounded up.  Measured on an MI355X with
# tests/test_gpu_regimes.py::test_one_step_matches_oracle (48 x 40, 60 iterations; it prints the ratio of
# every case): the worst field of the 28 cases at 0.85 ... 1.154 x the floor (largest: low-amp0.001-small
# 1.154, magic-amp0.03-big 1.127, Re100-amp0.03-small 1.111; per pair Re1 <= 1.03, Re10 <= 1.07,
# Re100 <= 1.11, BGK <= 1.06, swapped <= 1.05, magic <= 1.13, low <= 1.15), the populations <= 1.13 x;
# the deep sweeps of the default schedule on 70 x 125 and 3 x 130 over 17 iterations <= 1.165 x (populations
# <= 1.24 x).  The GPU rounds as the emulation does but for the reciprocal and fma ties, so it lands on
# the floor.  2 x 1.154 = 2.31 -> 3.  With the floor at 8.8e-7 ... 6.5e-6 the bound is <= 2e-5, and the
# smallest of the six seeded errors' best cases is 1524 x its floor (test_regimes_discriminate needs 3 x FACTOR).
FACTOR = 3

TAUS = {
    "Re1": reference_taus(1),            # (2.8068, 0.5361): the suite's pair, w+ < 1 < w-
    "Re10": reference_taus(10),          # (0.7307, 0.8613)
    "Re100": reference_taus(100),        # (0.5231, 4.1125): w- < 1 < w+
    "BGK": (0.8, 0.8),
    "swapped": reference_taus(1)[::-1],  # (0.5361, 2.8068)
    "magic": (1.0, 0.875),               # omp = 1 - w+ = 0 exactly
    "low": (0.51, 0.51),
}
AMPS = (1e-3, 3e-2)
FORCES = {"small": (1e-6, 0.0), "big": (1e-4, -5e-5)}
IB_AMP = {1e-3: 1.5e-3, 3e-2: 2e-2}  # IB point speed that goes with a state amplitude

Case = namedtuple("Case", "id name tau tau2 amp force ib_amp")


def case(name, amp, force):
    tau, tau2 = TAUS[name]
    return Case(f"{name}-amp{amp:g}-{force}", name, tau, tau2, amp, FORCES[force], IB_AMP[amp])


FULL = [case(n, a, f) for n, a, f in itertools.product(TAUS, AMPS, FORCES)]
CORNERS = [case("Re100", 3e-2, "big"), case("swapped", 3e-2, "big"), case("BGK", 3e-2, "small"),
           case("Re10", 1e-3, "big"), case("Re1", 3e-2, "big"), case("magic", 3e-2, "big")]
TODAY = case("Re1", 1e-3, "small")  # where every earlier parity test runs
PAIRS_BOTH_AMPS = [case(n, a, "small") for n, a in itertools.product(TAUS, AMPS)]

ids = lambda cases: [c.id for c in cases]

SHAPE, STEPS, SEED = (48, 40), 60, 7  # the one-step tests' lattice


def state(c, nx, ny, seed=SEED):
    return W.perturbed_state(nx, ny, seed, c.amp)


def line(xs, n, y0=3.0, dy=1.0, amp=1.5e-3):
    """A standing line of n points with speeds up to amp, every seventh masked (the _line of
    tests/test_gpu_fused.py)."""
    k = np.arange(n)
    s = np.empty(2 * n, dtype=np.float32)
    s[0::2] = xs + 0.25 * np.sin(0.3 * k)
    s[1::2] = y0 + dy * k
    us = np.zeros(2 * n, dtype=np.float32)
    us[0::2] = amp * (k / n)
    us[1::2] = -0.3 * amp * np.cos(0.2 * k)
    return s, us, (k % 7 != 3).astype(np.int32)


def edge_points(nx, amp):
    """points(it): the moving points of test_gpu_fused.py::test_ib_edges_and_epsilon (at x ~ 0 and
    x ~ XDIM, every fifth masked) with their speeds scaled by amp / 1.5e-3."""
    sc = amp / 1.5e-3

    def pts(it):
        ns = 30
        k = np.arange(ns)
        s = np.empty(2 * ns, dtype=np.float32)
        s[0::2] = np.where(k % 2 == 0, 0.2 + 0.01 * it, nx - 0.3 - 0.01 * it)
        s[1::2] = 2.0 + 3.0 * k
        us = np.zeros(2 * ns, dtype=np.float32)
        us[0::2] = sc * 1e-3 * np.sin(0.1 * it + k)
        us[1::2] = sc * 5e-4 * np.cos(0.1 * it)
        return s, us, (k % 5 != 0).astype(np.int32)
    return pts


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = float(np.max(np.abs(b))) if b.size else 0.0
    return (float(np.max(np.abs(a - b))) if a.size else 0.0) / (m if m > 0 else 1.0)


def field_errors(rho, u, rho_ref, u_ref):
    """max|x - ref| / max|ref| of rho - 1, u_x, u_y."""
    n = rho_ref.size
    return {"rho-1": rel(rho - 1, rho_ref - 1), "ux": rel(u[:n], u_ref[:n]), "uy": rel(u[n:], u_ref[n:])}


@functools.lru_cache(maxsize=None)
def oracle_run(O, c, nx, ny, steps, seed=SEED, flux_column=None, flux_norm=192.0):
    """The oracle's state after `steps` iterations without IB (shared by the tests; treat as read-only),
    and flux_scale = sum over the iterations of YDIM max|u_x| / flux_norm: what the flux sums, taken at the
    magnitude the u_x metric is relative to."""
    rho, u = state(c, nx, ny, seed)
    sim = O.Simulation(nx, ny, c.tau, c.tau2, rho=rho, u=u, body_force=c.force, flux_norm=flux_norm,
                       **({} if flux_column is None else {"flux_column": flux_column}))
    scale = 0.0
    for _ in range(steps):
        sim.step(1)
        scale += ny * float(np.max(np.abs(sim.u[:nx * ny]))) / flux_norm
    sim.flux_scale = scale
    return sim


def emulate(O, c, nx, ny, steps, seed=SEED, dtype=np.float32, mutate=None):
    """Field errors of the f32 collide's CPU emulation against the oracle."""
    from f32_gpu_model import F32GpuChannel
    sim = oracle_run(O, c, nx, ny, steps, seed)
    rho, u = state(c, nx, ny, seed)
    m = F32GpuChannel(nx, ny, c.tau, c.tau2, rho, u, c.force, dtype=dtype, mutate=mutate)
    m.step(steps)
    r, v = m.macro()
    return field_errors(r, v, sim.rho, sim.u)


@functools.lru_cache(maxsize=None)
def floor(O, c, nx=SHAPE[0], ny=SHAPE[1], steps=STEPS, seed=SEED):
    return max(emulate(O, c, nx, ny, steps, seed).values())


def f32_bound(O, c, nx=SHAPE[0], ny=SHAPE[1], steps=STEPS, seed=SEED):
    """The f32 bound without IB on rho - 1, u_x, u_y for a case, shape and iteration count."""
    b = FACTOR * floor(O, c, nx, ny, steps, seed)
    assert b <= TOL32, (c.id, b)  # never looser than the project's f32 bound
    return b


# ---- the immersed-boundary paths ------------------------------------------------------------------------
# The suite's bounds with IB (the band tests': test_gpu_fused.py::test_ib_band_cycle_matches_oracle).  The f32
# row is what every f32 IB path was held to before f32_ib_bound, and what f32_ib_bound may never exceed.
IB_TOL = {"f64": {"fields": 1e-10, "force": 1e-9, "F_s": 1e-5, "flux": 1e-9},
          "f32": {"fields": TOL32, "force": 1e-3, "F_s": 1e-2, "flux": 1e-4}}
IB_QUANTITIES = ("rho-1", "ux", "uy", "force", "F_s")
IB_TOL_OF = {"rho-1": "fields", "ux": "fields", "uy": "fields", "force": "force", "F_s": "F_s"}

# The two GPU configurations, by the name of their points: (XDIM, YDIM, iterations, state seed).
#   "edge": edge_points given every iteration (the IB one-step path, the local slab group);
#   "line": line(100.0, 40) given once (the band cycle: 3K + 2 iterations at the default depth K = 7).
IB_CONFIGS = {"edge": (64, 192, 30, SEED), "line": (256, 128, 23, 11)}
IB_CASES = CORNERS + [TODAY]

# FACTOR_IB = 2 x the largest GPU error / emulation floor over IB_CASES, every quantity and every f32 IB
# path, rounded up (the recipe of FACTOR).  Measured on an MI355X with tests/test_gpu_regimes.py (every test
# prints floor, error and ratio per quantity); error / floor over the 7 cases, smallest ... largest, and the
# largest per quantity (rho - 1, u_x, u_y, force, F_s):
#   one-step path (ib_point_kernel), edge      0.83 ... 1.50    1.17 1.18 1.25 1.00 1.50
#   band cycle, chained (ib_ghost_kernel)      0.80 ... 1.35    1.03 1.35 1.15 1.26 1.20
#   band cycle, merged (ib_next_group)         the chained cycle's figures, digit for digit
#   band cycle as the library picks it, and the same call on the one-step path: the same again
#   three f32 slabs (ib_ghost_kernel), edge    the one-step path's figures, digit for digit
# The dense force lands on the floor itself in 12 of the 14 edge runs (ratio 1.000: the same float32 F_s,
# the same products).  The largest ratio, 1.50, is F_s at TODAY on the edge points: F_s is a float32, its error
# a whole number of ulps of the largest F_s, 2 in the emulation and 3 on the GPU.  Every path is below 2 x the
# floor, so nothing was widened: 2 x 1.50 = 3.0 -> 3.  The flux differs from the oracle's by <= 0.05 x its
# bound.  The smallest best ratio of the six seeded errors is 3.6e4 x its floor, the smallest ratio in any
# single run where an error can show 210 (test_regimes_ib_discriminate needs 3 x FACTOR_IB = 9).
FACTOR_IB = 3


def ib_points(points, c, nx):
    """The points of a configuration at the case's IB speed: points(it), or one tuple given once."""
    assert points in IB_CONFIGS, points
    return edge_points(nx, c.ib_amp) if points == "edge" else line(100.0, 40, amp=c.ib_amp)


@functools.lru_cache(maxsize=None)
def ib_oracle_run(O, c, nx, ny, steps, points):
    """The oracle's state after `steps` iterations of a configuration (shared by the tests; treat as
    read-only), with flux_scale as oracle_run's."""
    pts = ib_points(points, c, nx)
    rho, u = state(c, nx, ny, IB_CONFIGS[points][3])
    sim = O.Simulation(nx, ny, c.tau, c.tau2, rho=rho, u=u, body_force=c.force)
    if not callable(pts):
        sim.set_lagrangian(*pts)
    scale = 0.0
    for it in range(steps):
        if callable(pts):
            sim.set_lagrangian(*pts(it))
        sim.step(1)
        scale += ny * float(np.max(np.abs(sim.u[:nx * ny]))) / 192.0
    sim.flux_scale = scale
    return sim


def _permutation(spread_order, ns):
    """spread_order of ib_run: None (the points' order), "reversed", or the seed of a permutation."""
    if spread_order is None:
        return None
    return np.arange(ns)[::-1] if spread_order == "reversed" else np.random.default_rng(spread_order).permutation(ns)


@functools.lru_cache(maxsize=None)
def ib_run(c, nx, ny, steps, points, dtype=np.float32, mutate=None, spread_order=None, perturb=None):
    """The IB emulation's readers after `steps` iterations of a configuration (treat as read-only)."""
    from f32_gpu_model import F32GpuIBChannel
    pts = ib_points(points, c, nx)
    ns = (pts(0) if callable(pts) else pts)[0].size // 2
    rho, u = state(c, nx, ny, IB_CONFIGS[points][3])
    m = F32GpuIBChannel(nx, ny, c.tau, c.tau2, rho, u, c.force, pts, dtype=dtype, mutate=mutate,
                        spread_order=_permutation(spread_order, ns), perturb=perturb)
    m.step(steps)
    r, v = m.macro()
    return {"rho": r, "u": v, "force": m.force(), "F_s": m.lagrangian_force()}


def ib_errors(rho, u, force, F_s, ref_rho, ref_u, ref_force, ref_F_s):
    """The metrics of the GPU tests' _check_ib: max|x - ref| / max|ref| of rho - 1, u_x, u_y, the dense
    force (with the body force) and F_s."""
    return {**field_errors(rho, u, ref_rho, ref_u), "force": rel(force, ref_force), "F_s": rel(F_s, ref_F_s)}


def ib_emulate(O, c, nx, ny, steps, points, dtype=np.float32, mutate=None, spread_order=None, perturb=None):
    """Errors of the IB emulation against the oracle, per quantity."""
    sim = ib_oracle_run(O, c, nx, ny, steps, points)
    out = ib_run(c, nx, ny, steps, points, dtype, mutate, spread_order, perturb)
    return ib_errors(out["rho"], out["u"], out["force"], out["F_s"], sim.rho, sim.u, sim.force, sim.F_s)


def ib_floor(O, c, nx, ny, steps, points):
    """The float32 IB emulation against the oracle, per quantity: what float32 costs on that path."""
    return ib_emulate(O, c, nx, ny, steps, points)


def _ib_difference(c, nx, ny, steps, points, **knobs):
    a, b = ib_run(c, nx, ny, steps, points, **knobs), ib_run(c, nx, ny, steps, points)
    return ib_errors(a["rho"], a["u"], a["force"], a["F_s"], b["rho"], b["u"], b["force"], b["F_s"])


ORDER_SEED = 5


def ib_order_envelope(c, nx, ny, steps, points):
    """What the arrival order of the spread atomics can change, per quantity: the float32 emulation against
    itself with the cast force (float)(g + F) of every forced cell moved by one float32 ulp, seeded signs, in
    every iteration.  (A cell's dense force is a double sum of a few terms; another order moves it by ~1e-16
    of itself, which the cast to float32 turns into at most one ulp.)"""
    return _ib_difference(c, nx, ny, steps, points, perturb=ORDER_SEED)


def ib_order_spread(c, nx, ny, steps, points):
    """The largest difference, per quantity, among the emulation with the points' terms reaching each cell
    in reversed order and in three seeded orders, against the points' own order."""
    runs = [_ib_difference(c, nx, ny, steps, points, spread_order=o) for o in ("reversed", 1, 2, 3)]
    return {q: max(r[q] for r in runs) for q in IB_QUANTITIES}


def f32_ib_bound(O, c, nx, ny, steps, points):
    """The f32 bounds with IB, per quantity: FACTOR_IB x the emulation's floor for the case and configuration."""
    b = {q: FACTOR_IB * v for q, v in ib_floor(O, c, nx, ny, steps, points).items()}
    for q, v in b.items():
        assert v <= IB_TOL["f32"][IB_TOL_OF[q]], (c.id, points, q, v)  # never looser than the earlier bound
    return b
