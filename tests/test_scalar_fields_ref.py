"""tests/scalar_fields_ref.py on the CPU: the wall flux it restates is the scalar's budget.  Over one substep of
tests/scalar_ref.py the sum over x of bottom + top equals the change of sum(C), for value walls on both sides, a
value wall below a no-flux wall, and two no-flux walls (exact zeros).  The GPU tests
(tests/test_gpu_scalar_fields.py) compare the device with this restatement bit for bit; this test shows that the
restatement is the flux it claims to be.

Bound: 4 * N * 2^-53 * sum|g| with N the cell count, the rounding bound of the sums involved: a sum of n doubles
taken in any order is within n * 2^-53 * sum|x| of exact (Higham §4.2), and the two totals and the substep's own
relaxation (whose roundings the identity does not see) involve the 5 N populations a few times over.  The totals
here are taken with math.fsum of the cells' C, so what is observed is far smaller (it is printed).
"""
import math

import numpy as np
import pytest

import scalar_fields_ref as F
import scalar_ref as S

NX, NY, TAU = 12, 9, 0.8
WALLS = {
    "value / value": ((S.VALUE, 0.25), (S.VALUE, 1.75)),
    "value / no flux": ((S.VALUE, 0.25), (S.NOFLUX, 0.0)),
    "no flux / no flux": S.NO_FLUX_WALLS,
}


def seeded_state():
    rng = np.random.default_rng(12)
    ux, uy = 0.05 * rng.uniform(-1.0, 1.0, (NY, NX)), 0.05 * rng.uniform(-1.0, 1.0, (NY, NX))
    C0 = rng.uniform(0.5, 1.5, (NY, NX))
    return S.equilibrium(C0, ux, uy), ux, uy


@pytest.mark.parametrize("walls", list(WALLS))
def test_the_wall_flux_is_the_change_of_the_total(walls):
    g, ux, uy = seeded_state()
    total = lambda g: math.fsum(S.concentration(g).ravel())
    moved = 0.0
    for k in range(5):
        before = total(g)
        g = S.substep(g, ux, uy, TAU, WALLS[walls])
        bottom, top = F.wall_flux(g, WALLS[walls])
        assert bottom.shape == top.shape == (NX,)
        flux = math.fsum(np.concatenate([bottom, top]))
        change = total(g) - before
        bound = 4 * NX * NY * 2.0 ** -53 * math.fsum(np.abs(g).ravel())
        print(f"{walls}, substep {k}: flux {flux:.17g} change {change:.17g} |diff| {abs(flux - change):.3e} bound {bound:.3e}")
        assert abs(flux - change) <= bound
        for (kind, _), side in zip(WALLS[walls], (bottom, top)):
            if kind == S.NOFLUX:
                assert np.all(side == 0.0) and not np.any(np.signbit(side))
            else:
                assert np.all(side != 0.0)
        moved = max(moved, abs(change))
    # the case is not empty: a value wall moved the total by far more than the bound
    assert (moved > 1e-3) == (walls != "no flux / no flux")


def test_the_fields_are_the_stated_products():
    g, ux, uy = seeded_state()
    f = F.scalar_fields(g, ux, uy)
    assert list(f) == ["c", "cux", "cuy"]
    assert np.array_equal(f["c"], (((g[0] + g[1]) + g[2]) + g[3]) + g[4])
    assert np.array_equal(f["cux"], f["c"] * ux) and np.array_equal(f["cuy"], f["c"] * uy)
    g[2, 3, 4] = np.nan
    f = F.scalar_fields(g, ux, uy)
    for n in f:
        assert np.isnan(f[n][3, 4]) and np.isfinite(np.delete(f[n].ravel(), 3 * NX + 4)).all()
