"""CPU side of the regime tests (tests/regimes.py): the cases are stable in the oracle, the f32 collide's
emulation (tests/f32_gpu_model.py) stays at its floor in every one of them, and the bound the GPU tests
assert (regimes.f32_bound) separates a collide that is wrong in one nonlinear or forcing term from a
right one — which the suite's earlier f32 assertion, at its one regime, does not.
"""
import numpy as np

import regimes as R
from f32_gpu_model import MUTATIONS

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

