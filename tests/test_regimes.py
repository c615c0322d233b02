"""CPU side of the regime tests (tests/regimes.py): the cases are stable in the oracle, the f32 collide's
emulation (tests/f32_gpu_model.py) stays at its floor in every one of them, and the bound the GPU tests
assert (regimes.f32_bound) separates a collide that is wrong in one nonlinear or forcing term from a
right one — which the suite's earlier f32 assertion, at its one regime, does not.  The same for the f32
immersed-boundary paths: the IB iteration's emulation (F32GpuIBChannel) is the oracle's algorithm in double,
its float32 floors, what the arrival order of the spread can change, and six seeded IB errors against the
bound regimes.f32_ib_bound.
"""
import numpy as np

import regimes as R
from f32_gpu_model import IB_MUTATIONS, MUTATIONS

MARGIN = 1.5  # on magnitudes measured once from the seeded states (deterministic)


def test_regimes_oracle_bounded(oracle):
    """Every case stays finite and small in the oracle: no-IB at 48 x 40 over 60 iterations (measured:
    max|rho - 1| 3.3e-2, max|u| 3e-2), and every relaxation pair at both amplitudes with a 40-point line
    at 256 x 128 over 23 iterations, the band tests' configuration (measured: max|rho - 1| 4.1e-2,
    max|u| 2.9e-2 without the pair `low`, 4.9e-2 and 4.3e-2 with it; the IB force starts at 3.1e-2 and
    decays)."""
    for c in R.FULL:
        sim = R.oracle_run(oracle, c, *R.SHAPE, R.STEPS)
        assert np.isfinite(sim.f).all() and np.isfinite(sim.u).all(), c.id
        assert np.max(np.abs(sim.rho - 1)) <= MARGIN * 3.3e-2, c.id
        assert np.max(np.abs(sim.u)) <= MARGIN * 3e-2, c.id
    nx, ny = 256, 128
    for c in R.PAIRS_BOTH_AMPS:
        rho, u = R.state(c, nx, ny, 11)
        sim = oracle.Simulation(nx, ny, c.tau, c.tau2, rho=rho, u=u, body_force=c.force)
        sim.set_lagrangian(*R.line(100.0, 40, amp=c.ib_amp))
        fmax = []
        for _ in range(23):
            sim.step(1)
            fmax.append(float(np.max(np.abs(sim.force))))
        assert np.isfinite(sim.f).all() and np.isfinite(sim.force).all(), c.id
        assert np.max(np.abs(sim.rho - 1)) <= MARGIN * 4.1e-2, (c.id, np.max(np.abs(sim.rho - 1)))
        assert np.max(np.abs(sim.u)) <= MARGIN * 2.9e-2, (c.id, np.max(np.abs(sim.u)))
        assert max(fmax) <= MARGIN * 3.1e-2 and fmax[-1] < fmax[0], (c.id, fmax)


def test_regimes_f32_floor(oracle):
    """The unmutated emulation against the oracle on rho - 1, u_x, u_y in every FULL case: float32
    <= 1e-5 (measured maximum 6.5e-6), the same operation order in float64 <= 1e-10 (measured 3e-11)."""
    for c in R.FULL:
        e32 = R.floor(oracle, c)
        e64 = max(R.emulate(oracle, c, *R.SHAPE, R.STEPS, dtype=np.float64).values())
        assert e32 <= 1e-5, (c.id, e32)
        assert e64 <= 1e-10, (c.id, e64)
        assert R.f32_bound(oracle, c) <= R.TOL32


def test_regimes_discriminate(oracle):
    """The power of the GPU tests, without a GPU.  Each of six seeded errors of the f32 collide's
    nonlinear and forcing terms (f32_gpu_model.MUTATIONS) exceeds 3 x f32_bound in at least one FULL
    case; and M1, M3, M4, M6 pass the suite's earlier f32 assertion, max(rho, u_x, u_y) <= 1e-4 with rho
    normalised by max|rho| ~ 1, at its regime (Re1, amplitude 1e-3, force (1e-6, 0)): the gap these
    tests close."""
    for m in MUTATIONS:
        worst = {c.id: max(R.emulate(oracle, c, *R.SHAPE, R.STEPS, mutate=m).values()) / R.f32_bound(oracle, c)
                 for c in R.FULL}
        assert max(worst.values()) >= 3, (m, worst)
    c = R.TODAY
    sim = R.oracle_run(oracle, c, *R.SHAPE, R.STEPS)
    for m in ("M1", "M3", "M4", "M6"):
        e = R.emulate(oracle, c, *R.SHAPE, R.STEPS, mutate=m)
        e_rho = e["rho-1"] * float(np.max(np.abs(sim.rho - 1)) / np.max(np.abs(sim.rho)))
        assert max(e_rho, e["ux"], e["uy"]) <= R.TOL32, (m, e)


# ---- the immersed-boundary paths --------------------------------------------------------------------------
def _ib_configs():
    return [(points, nx, ny, steps) for points, (nx, ny, steps, _) in R.IB_CONFIGS.items()]


def test_ib_model_delta(oracle):
    """The emulation's vectorised d_delta equals the oracle's bit for bit: 4000 seeded (point, node) pairs
    in and around the kernel's support, with distances of exactly 0.5 and 1.5 among them."""
    from f32_gpu_model import d_delta
    rng = np.random.default_rng(0)
    xs, ys = rng.uniform(-1, 5, (2, 4000)).astype(np.float32)
    xs[:60] = np.tile(np.array([0.5, 1.5, 2.5, 3.0, 2.0], np.float32), 12)
    x, y = rng.integers(-2, 6, (2, 4000))
    ref = np.array([oracle.d_delta(float(a), float(b), int(i), int(j)) for a, b, i, j in zip(xs, ys, x, y)], np.float32)
    mine = d_delta(xs, ys, x, y)
    assert np.count_nonzero(ref) > 400
    assert np.array_equal(mine, ref)


# floors measured once (deterministic): the largest over IB_CASES of fields (rho - 1, u_x, u_y), force, F_s
IB_FLOOR_MAX = {"edge": {"fields": 1.66e-6, "force": 7.20e-7, "F_s": 5.23e-7},
                "line": {"fields": 1.30e-6, "force": 1.20e-6, "F_s": 9.94e-7}}


def test_regimes_ib_floor(oracle):
    """The IB emulation against the oracle in every case of CORNERS + [TODAY], in the two GPU configurations
    (64 x 192, 30 iterations, edge_points per iteration; 256 x 128, 23 iterations, line(100.0, 40)).

    The float64-order emulation meets the project's f64 IB bounds (fields 1e-10, force 1e-9, F_s 1e-5), so
    the emulation is the oracle's algorithm.  Measured: fields <= 1.42e-12, the dense force and F_s equal to
    the oracle's bit for bit in all 14 runs.

    The float32 emulation's floors, measured maxima (asserted with MARGIN):
      edge  rho - 1 1.66e-6 (BGK), u_x 1.40e-6, u_y 1.53e-6, force 7.20e-7, F_s 5.23e-7
      line  rho - 1 1.06e-6, u_x 1.09e-6, u_y 1.30e-6 (magic), force 1.20e-6 (Re10), F_s 9.94e-7
    and FACTOR_IB x floor never exceeds the earlier f32 bound (f32_ib_bound asserts it): at most 5e-6 on the
    fields against 1e-4, 3.6e-6 on the force against 1e-3, 3e-6 on F_s against 1e-2."""
    tol = R.IB_TOL["f64"]
    for points, nx, ny, steps in _ib_configs():
        for c in R.IB_CASES:
            e64 = R.ib_emulate(oracle, c, nx, ny, steps, points, dtype=np.float64)
            for q, v in e64.items():
                assert v <= tol[R.IB_TOL_OF[q]], (points, c.id, q, v)
            e32 = R.ib_floor(oracle, c, nx, ny, steps, points)
            for q, v in e32.items():
                assert 0 < v <= MARGIN * IB_FLOOR_MAX[points][R.IB_TOL_OF[q]], (points, c.id, q, v)
            R.f32_ib_bound(oracle, c, nx, ny, steps, points)


def test_regimes_ib_order_envelope():
    """What the arrival order of the spread atomics can do to an f32 run: ib_order_envelope (every forced
    cell's cast force one float32 ulp off, seeded signs, every iteration) against the largest difference
    among the emulation's runs with reversed and three seeded spread orders.

    Measured per case, envelope (rho - 1, u_x, u_y | force, F_s); the orders' largest difference is 0 in
    every one of the 14 runs (edge_points' stencils do not overlap; the line's do, by up to three terms per
    cell, and the double sums then differ by ~1e-16 of themselves, which never crosses a float32 rounding
    boundary of (float)(g + F) in these runs):
               edge                                        line
      Re100    2.4e-7 2.1e-7 2.0e-7 | 1.5e-7 9.4e-8        2.2e-7 1.7e-7 1.8e-7 | 1.8e-7 1.7e-7
      swapped  2.8e-7 1.8e-7 1.3e-7 | 1.6e-7 9.4e-8        2.8e-7 1.5e-7 1.3e-7 | 1.4e-7 1.2e-7
      BGK      1.4e-7 1.2e-7 1.2e-7 | 1.1e-7 5.5e-8        2.0e-7 1.4e-7 1.3e-7 | 2.6e-7 2.1e-7
      Re10     2.9e-7 1.6e-7 2.2e-7 | 1.2e-7 5.8e-8        2.3e-7 1.7e-7 2.4e-7 | 1.3e-7 9.5e-8
      Re1      1.8e-7 3.0e-7 2.6e-7 | 8.8e-8 6.4e-8        2.4e-7 3.4e-7 3.3e-7 | 2.0e-7 1.9e-7
      magic    1.8e-7 9.5e-8 1.1e-7 | 5.1e-8 5.9e-8        1.8e-7 1.3e-7 1.9e-7 | 2.0e-7 1.6e-7
      TODAY    2.6e-7 3.1e-7 2.8e-7 | 9.3e-8 8.8e-8        2.0e-7 2.8e-7 3.7e-7 | 1.6e-7 1.2e-7
    The envelope is of the floor's own size (0.1 ... 1.3 x): an f32 run is only defined up to it."""
    for points, nx, ny, steps in _ib_configs():
        for c in R.IB_CASES:
            env = R.ib_order_envelope(c, nx, ny, steps, points)
            spread = R.ib_order_spread(c, nx, ny, steps, points)
            print("REGIME ib_order", points, c.id, " ".join(f"{q}={env[q]:.2e}/{spread[q]:.2e}" for q in env))
            for q in env:
                assert 0 < env[q] <= 1e-6, (points, c.id, q, env[q])  # ulp-sized: a few float32 roundings
                assert spread[q] <= env[q], (points, c.id, q, spread[q], env[q])


# What the earlier f32 bounds (IB_TOL["f32"]: fields 1e-4, force 1e-3, F_s 1e-2) let through at TODAY, per
# seeded error: the quantities whose error stays within its earlier bound in every configuration where the
# error can show (see test_regimes_ib_discriminate).
IB_PASSED_TODAY = {"I1": {"F_s"}, "I2": {"force", "F_s"}, "I3": {"force", "F_s"}, "I4": set(), "I5": set(),
                   "I6": {"F_s"}}


def test_regimes_ib_discriminate(oracle):
    """The power of the f32 IB assertions of tests/test_gpu_regimes.py, without a GPU: each of the six seeded
    one-term errors of the IB iteration (f32_gpu_model.IB_MUTATIONS) exceeds 3 x FACTOR_IB x floor in at
    least one quantity of at least one case (all six do).  Best ratio error / floor per error, over the 14
    runs: I1 2.0e5 (u_y, edge, Re10), I2 3.6e4 (rho - 1, edge, Re1-amp0.03), I3 4.9e4 (force, line, Re100),
    I4 5.6e5 (F_s, edge, TODAY), I5 2.9e6 (u_y, edge, TODAY), I6 9.6e4 (force, edge, TODAY); the smallest
    ratio of an error's best quantity in any run where it can show is 210 (I1, BGK, small body force).  I4 and
    I6 cannot show on the standing line away from the x edges, where they leave every bit unchanged; the
    moving edge_points show both in every case.

    The gap.  At TODAY the earlier bounds saw none of the six in the dense force's or F_s's own assertion
    where IB_PASSED_TODAY names them: I2 and I3 leave both within 1e-3 / 1e-2 (I3: force 1.5e-4 ... 4.0e-4,
    F_s 1.7e-4 ... 3.5e-4), I1 and I6 leave F_s within 1e-2 (2.3e-3, 3.1e-3).  What caught them was the fields' 1e-4 alone,
    I3 by a factor of 1.8 (edge: rho - 1 1.78e-4, u_x 1.38e-4, u_y 1.28e-4).  The new bound sees every
    quantity named there at more than 3 x FACTOR_IB x its floor."""
    old = R.IB_TOL["f32"]
    best = {m: 0.0 for m in IB_MUTATIONS}
    passed = {m: set(R.IB_QUANTITIES) for m in IB_MUTATIONS}
    for points, nx, ny, steps in _ib_configs():
        for c in R.IB_CASES:
            fl = R.ib_floor(oracle, c, nx, ny, steps, points)
            for m in IB_MUTATIONS:
                e = R.ib_emulate(oracle, c, nx, ny, steps, points, mutate=m)
                best[m] = max(best[m], max(e[q] / fl[q] for q in e))
                if c == R.TODAY and any(e[q] != fl[q] for q in e):  # (where the error can show)
                    passed[m] &= {q for q in e if e[q] <= old[R.IB_TOL_OF[q]]}
                    for q in IB_PASSED_TODAY[m]:
                        assert e[q] <= old[R.IB_TOL_OF[q]], (m, points, q, e[q])
                        assert e[q] >= 3 * R.FACTOR_IB * fl[q], (m, points, q, e[q], fl[q])
    print("REGIME ib_discriminate", " ".join(f"{m}={v:.3g}" for m, v in best.items()))
    assert all(v >= 3 * R.FACTOR_IB for v in best.values()), best
    assert {m: {q for q in s if R.IB_TOL_OF[q] != "fields"} for m, s in passed.items()} == IB_PASSED_TODAY, passed

