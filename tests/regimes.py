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
at its definition below).  f32 with IB (no emulation of that path): TOL32 = 1e-4
on rho - 1, u_x, u_y, force 1e-3, F_s 1e-2, flux 1e-4.
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
