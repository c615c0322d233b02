"""tests/particle_ref.py checked on the CPU: the hash against a big-integer restatement, the range and the
variance of the random step, the zero model against tracer_ref.advect, and every wall kind on hand-built steps."""
import numpy as np
import pytest

import particle_ref as P
import tracer_ref as T

MASK = (1 << 64) - 1


def py_mix(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def py_raw(seed, p, m, k):
    key = py_mix((seed + 0x9E3779B97F4A7C15 * (p + 1)) & MASK)
    return py_mix((key + 0x9E3779B97F4A7C15 * (2 * m + k + 1)) & MASK)


@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEFCAFEF00D, MASK])
def test_the_hash_equals_a_big_integer_restatement(seed):
    for p in (0, 1, 63, 999, 2**31 + 5):
        for m in (0, 1, 7, 10**9):
            for k in (0, 1):
                r = py_raw(seed, p, m, k)
                assert int(P.raw(seed, np.array([p]), m, k)[0]) == r, (seed, p, m, k)
                assert P.xi(seed, np.array([p]), m, k)[0] == (r >> 11) / 2.0**52 - 1.0
    # an array of tracers is the scalars side by side
    got = P.raw(seed, np.arange(5), 3, 1)
    assert [int(v) for v in got] == [py_raw(seed, p, 3, 1) for p in range(5)]


def test_xi_lies_in_the_half_open_interval():
    p = np.arange(20000)
    for m in (0, 5):
        for k in (0, 1):
            v = P.xi(12345, p, m, k)
            assert v.dtype == np.float64 and np.all(v >= -1.0) and np.all(v < 1.0)
            assert abs(v.mean()) < 5 / np.sqrt(3 * p.size)  # uniform: variance 1/3
    # the extremes of the map itself
    assert (np.uint64(0) >> np.uint64(11)).astype(np.float64) * 2.0**-52 - 1.0 == -1.0
    assert (np.uint64(MASK) >> np.uint64(11)).astype(np.float64) * 2.0**-52 - 1.0 == 1.0 - 2.0**-52
    # x and y, consecutive updates and neighbouring tracers draw different numbers
    a = P.xi(7, p, 0, 0)
    for other in (P.xi(7, p, 0, 1), P.xi(7, p, 1, 0), P.xi(8, p, 0, 0), np.roll(a, 1)):
        assert abs(np.corrcoef(a, other)[0, 1]) < 5 / np.sqrt(p.size)


@pytest.mark.parametrize("D,stride,M", [(0.05, 3, 20), (0.02, 5, 24), (0.3, 1, 50)])
def test_the_displacement_variance_is_2_D_stride_M(D, stride, M):
    n, nx, ny = 4000, 64, 4001  # zero velocity, the walls 2000 rows away: at most amp * M < 100 rows are crossed
    zero = np.zeros(n)
    x0, y0 = np.full(n, 32.0), np.full(n, 2000.0)
    x, y, laps, st, hit = x0, y0, np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int64)
    for m in range(M):
        x, y, laps, st, hit, _ = P.step(zero, zero, x, y, laps, st, hit, stride, m, (m + 1) * stride, (nx, ny),
                                        diffusivity=D, walls=(P.ABSORB, P.ABSORB), seed=99)
    assert not st.any() and np.all(hit == -1)
    want = 2.0 * D * stride * M
    bound = 5.0 * np.sqrt(2.0 / (n - 1))  # five standard errors of a sample variance
    for name, d in (("x", x - x0 + laps * float(nx)), ("y", y - y0)):
        var = d.var(ddof=1)
        print(f"D {D} stride {stride} M {M} {name}: variance {var:.5f} expected {want:.5f} rel {var / want - 1:+.4f} bound {bound:.4f}")
        assert abs(var / want - 1.0) <= bound, (name, var, want)
        assert abs(d.mean()) <= 5.0 * np.sqrt(want / n), (name, d.mean())


def test_the_zero_model_is_the_plain_rule():
    rng = np.random.default_rng(5)
    nx, ny, n = 20, 18, 400
    ux, uy = rng.normal(0, 0.4, (ny, nx)), rng.normal(0, 0.4, (ny, nx))  # fast: wraps and clamps happen
    ux[4, 7] = np.nan
    sx, sy = T.special_points(nx, ny)
    x = np.concatenate([sx, rng.uniform(0, nx, n)])
    y = np.concatenate([sy, rng.uniform(0, ny - 1, n)])
    x[x >= nx] = 0.0
    laps, st, hit = np.zeros(x.size, np.int32), np.zeros(x.size, np.int32), np.full(x.size, -1, np.int64)
    wrapped = clamped = stayed = False
    for m, stride in enumerate((1, 3, 8, 60)):
        want = T.advect(ux, uy, x, y, laps, stride)
        got = P.advect(ux, uy, x, y, laps, st, hit, stride, m, 10 * m, seed=4)
        wrapped |= bool(np.any(want[2] != laps))
        clamped |= bool(np.any((want[1] == 0.0) & (y > 0)) and np.any((want[1] == ny - 1.0) & (y < ny - 1)))
        stayed |= bool(np.any(want[0] == x))
        for a, b in zip(got[:3], want):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert not got[3].any() and np.all(got[4] == -1) and not got[5].any()
        x, y, laps = want
    assert wrapped and clamped and stayed


def one(x, y, su, sv, shape=(20, 18), status=0, hit=-1, laps=0, stride=1, t=7, **model):
    """One hand-built tracer through one update: (x, y, laps, status, hit, reflected) as Python scalars."""
    r = P.step(np.array([su]), np.array([sv]), np.array([x]), np.array([y]), np.array([laps], np.int32),
               np.array([status], np.int32), np.array([hit], np.int64), stride, 0, t, shape, **model)
    return tuple(v[0].item() for v in r)


def test_clamp():
    assert one(3.0, 0.5, 0.25, -2.0) == (3.25, 0.0, 0, 0, -1, False)
    assert one(3.0, 16.5, 0.25, 2.0) == (3.25, 17.0, 0, 0, -1, False)
    assert one(3.0, 0.0, 0.25, -2.0) == (3.25, 0.0, 0, 0, -1, False)  # a start on the wall's row


def test_reflect():
    R = dict(walls=(P.REFLECT, P.REFLECT))
    assert one(3.0, 0.5, 0.25, -2.0, **R) == (3.25, 1.5, 0, 0, -1, True)
    assert one(3.0, 16.5, 0.25, 2.0, **R) == (3.25, 15.5, 0, 0, -1, True)
    assert one(3.0, 0.0, 0.25, -2.0, **R) == (3.25, 2.0, 0, 0, -1, True)  # a start on the wall's row
    assert one(3.0, 17.0, 0.25, 0.5, **R) == (3.25, 16.5, 0, 0, -1, True)
    # an overshoot past the opposite wall: folded back, then clamped
    assert one(3.0, 0.5, 0.25, -40.0, **R) == (3.25, 17.0, 0, 0, -1, True)
    assert one(3.0, 16.5, 0.25, 40.0, **R) == (3.25, 0.0, 0, 0, -1, True)
    # one wall reflects, the other clamps
    assert one(3.0, 16.5, 0.25, 2.0, walls=(P.REFLECT, P.CLAMP)) == (3.25, 17.0, 0, 0, -1, False)
    # inside: untouched
    assert one(3.0, 8.0, 0.25, 2.0, **R) == (3.25, 10.0, 0, 0, -1, False)


def test_absorb():
    A = dict(walls=(P.ABSORB, P.ABSORB))
    # half of the step is above the wall: lam = 0.5
    assert one(3.0, 1.0, 0.5, -2.0, **A) == (3.25, 0.0, 0, P.AT_BOTTOM, 7, False)
    assert one(3.0, 16.0, 0.5, 2.0, **A) == (3.25, 17.0, 0, P.AT_TOP, 7, False)
    # a start on the wall's row: lam = 0, it deposits where it is
    assert one(3.0, 0.0, 0.5, -2.0, **A) == (3.0, 0.0, 0, P.AT_BOTTOM, 7, False)
    assert one(3.0, 17.0, 0.5, 2.0, **A) == (3.0, 17.0, 0, P.AT_TOP, 7, False)
    # a step that ends on the row exactly does not cross it
    assert one(3.0, 1.0, 0.5, -1.0, **A) == (3.5, 0.0, 0, P.ALIVE, -1, False)
    # a deposited tracer never moves again, whatever the velocity
    assert one(3.0, 0.0, 0.5, 2.0, status=P.AT_BOTTOM, hit=4, **A) == (3.0, 0.0, 0, P.AT_BOTTOM, 4, False)
    assert one(3.0, 17.0, 0.5, -2.0, status=P.AT_TOP, hit=4, laps=2, **A) == (3.0, 17.0, 2, P.AT_TOP, 4, False)
    # one wall absorbs, the other reflects
    assert one(3.0, 16.0, 0.5, 2.0, walls=(P.ABSORB, P.REFLECT)) == (3.5, 16.0, 0, 0, -1, True)


def test_a_step_across_the_seam_and_a_wall_at_once():
    # x crosses XDIM = 20: absorbed at lam = 0.5 before the seam (19.75), at lam = 0.75 past it (20.125 -> 0.125)
    A = dict(walls=(P.ABSORB, P.ABSORB))
    assert one(19.5, 1.0, 0.5, -2.0, **A) == (19.75, 0.0, 0, P.AT_BOTTOM, 7, False)
    assert one(19.75, 1.5, 0.5, -2.0, **A) == (0.125, 0.0, 1, P.AT_BOTTOM, 7, False)
    assert one(0.25, 15.5, -0.5, 2.0, **A) == (19.875, 17.0, -1, P.AT_TOP, 7, False)
    # reflect and clamp wrap on the full step
    assert one(19.75, 1.5, 0.5, -2.0, walls=(P.REFLECT, P.CLAMP)) == (0.25, 0.5, 1, 0, -1, True)
    assert one(19.75, 1.5, 0.5, -2.0) == (0.25, 0.0, 1, 0, -1, False)
    # more than one lattice length: x and laps stay, y and the status still take effect
    assert one(19.75, 1.0, 100.0, -2.0, **A) == (19.75, 0.0, 0, P.AT_BOTTOM, 7, False)
    assert one(19.75, 1.0, 100.0, -2.0, walls=(P.REFLECT, P.CLAMP)) == (19.75, 1.0, 0, 0, -1, True)


def test_drift_and_a_non_finite_sample():
    # the drift is added to the fluid's velocity before the stride multiplies
    assert one(3.0, 8.0, 0.25, 0.5, stride=4, drift=(0.125, -0.25)) == (4.5, 9.0, 0, 0, -1, False)
    # a non-finite sample: unchanged and alive, even where the drift alone would cross an absorbing wall
    for su, sv in ((np.nan, 0.0), (0.0, np.inf)):
        assert one(3.0, 0.25, su, sv, drift=(0.0, -1.0), walls=(P.ABSORB, P.ABSORB)) == (3.0, 0.25, 0, 0, -1, False)


def test_a_large_diffusivity_keeps_every_position_in_range():
    nx, ny, n = 20, 18, 500
    rng = np.random.default_rng(2)
    x, y = rng.uniform(0, nx, n), rng.uniform(0, ny - 1, n)
    x[x >= nx] = 0.0
    zero = np.zeros(n)
    assert P.amplitude(300.0, 1) > ny
    r = P.step(zero, zero, x, y, np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int64), 1, 0, 1,
               (nx, ny), diffusivity=300.0, walls=(P.REFLECT, P.REFLECT), seed=1)
    assert np.all((r[0] >= 0) & (r[0] < nx) & (r[1] >= 0) & (r[1] <= ny - 1))
    assert np.any(r[0] == x) and np.any(r[0] != x)        # some steps exceed one lattice length, some do not
    assert np.any(r[5] & ((r[1] == 0.0) | (r[1] == ny - 1.0)))  # reflect, then clamp
