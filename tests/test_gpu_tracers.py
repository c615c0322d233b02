"""iblb_sample_points and the passive tracers on the GPU against tests/tracer_ref.py (checked on the CPU
by tests/test_tracer_ref.py) applied to what Lattice.fields returns for the same state.

Lattices 20 x 18 and 37 x 23 (an odd size, fewer rows than a wave), f64 and f32 storage, a seeded
perturbed state, a body force with both components and, where stated, the five Lagrangian points of
tests/test_gpu_fields.py.

Sampling and the trajectories without IB points are compared with `==`: the device evaluates the four
cells with the functions iblb_get_fields uses and interpolates with one rounding per operation, and the
host twin is stepped in exactly the pieces iblb_step cuts its calls into.  With moving IB points the
spread's atomic order may differ in the last bits between two contexts, so there the bound is
1e-9 * (path length of that tracer + 1): the project's f64 parity bound for u (tests/test_gpu_bulk.py),
accumulated over the path.  The twin lattices of the `==` comparisons carry no IB points for the same reason.
"""
import ctypes as C

import numpy as np
import pytest

import tracer_ref as T
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_fields import BODY_FORCE, points

pytestmark = pytest.mark.gpu

LATTICES = [(20, 18), (37, 23)]
PRECISIONS = ["f64", "f32"]
ALL = ["rho", "ux", "uy", "vort", "sxx", "sxy", "syy"]
COUNTS = [1, 63, 64, 65, 1000]


def new_lattice(gpu, nx, ny, precision, with_points=False, state=None, **kw):
    rho, u = state if state is not None else W.perturbed_state(nx, ny, 7)
    lat = gpu.Lattice(nx, ny, W.TAU, W.TAU2, precision=precision, body_force=BODY_FORCE,
                      max_points=8 if with_points else 0, **kw)
    lat.set_state(rho, u)
    if with_points:
        lat.set_lagrangian(*points(nx, ny))
    return lat


def point_set(nx, ny, n, seed=3):
    """n points: the special positions of tracer_ref first, then cell centres, then random interior points."""
    rng = np.random.default_rng(seed)
    sx, sy = T.special_points(nx, ny)
    ncen = min(max(n - sx.size, 0), 40)
    cx, cy = rng.integers(0, nx, ncen).astype(float), rng.integers(0, ny, ncen).astype(float)
    nr = max(n - sx.size - ncen, 0)
    rx, ry = rng.uniform(0, nx, nr), rng.uniform(0, ny - 1, nr)
    rx[rx >= nx] = 0.0
    x, y = np.concatenate([sx, cx, rx]), np.concatenate([sy, cy, ry])
    return x[:n], y[:n]


def pieces(t0, stride, t, calls):
    """The pieces iblb_step cuts `calls` into for tracers set at t0 (state at t now): [(iterations, update?)]."""
    out, nxt = [], t0 + stride
    while nxt <= t:
        nxt += stride
    for n in calls:
        while n > 0:
            p = min(n, nxt - t)
            t, n = t + p, n - p
            out.append((p, t == nxt))
            if t == nxt:
                nxt += stride
    return out


def host_trajectory(B, x, y, laps, stride, plan):
    """Step the twin B in the given pieces and update (x, y, laps) on the host; also every tracer's path length."""
    path = np.zeros_like(x)
    for n, update in plan:
        B.step(n)
        if update:
            f = B.fields(["ux", "uy"])
            xn, yn, ln = T.advect(f["ux"], f["uy"], x, y, laps, stride)
            dx = xn - x + (ln - laps) * float(B.nx)
            path += np.abs(dx) + np.abs(yn - y)
            x, y, laps = xn, yn, ln
    return x, y, laps, path


# ---- sampling -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_samples_equal_the_reference(gpu, nx, ny, precision):
    lat = new_lattice(gpu, nx, ny, precision, with_points=True)
    try:
        px, py = point_set(nx, ny, 1000)
        spec = T.special_points(nx, ny)[0].size
        for t in (0, 9):  # the boot phase, then a deep launch plus remainders
            if t:
                lat.step(t)
            full = lat.fields(ALL)
            if t:
                assert np.max(np.abs(full["sxy"])) > 0 and np.max(np.abs(full["vort"])) > 0
            for n in COUNTS:
                # n = 1: the last position below XDIM on the top row; the others start at the special positions
                x, y = (px[8:9], py[8:9]) if n == 1 else (px[:n], py[:n])
                assert n == 1 or n > spec
                got = lat.sample(ALL, x, y)
                ref = T.sample_fields(full, x, y)
                assert list(got) == ALL
                for name in ALL:
                    assert got[name].shape == (n,)
                    assert np.array_equal(got[name], ref[name]), (t, n, name, np.max(np.abs(got[name] - ref[name])))
            # a subset, given out of order: planes in ascending bit order
            sub = lat.sample(["uy", "rho"], px[:65], py[:65])
            assert list(sub) == ["rho", "uy"]
            for name in sub:
                assert np.array_equal(sub[name], T.sample(full[name], px[:65], py[:65])), (t, name)
        assert lat.sample("ux", [], [])["ux"].shape == (0,)
    finally:
        lat.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sampling_does_not_disturb_the_run(gpu, precision):
    nx, ny = LATTICES[1]
    a = new_lattice(gpu, nx, ny, precision)
    b = new_lattice(gpu, nx, ny, precision)
    try:
        px, py = point_set(nx, ny, 200)
        a.sample(ALL, px, py)
        a.step(3)
        b.step(3)
        a.sample(ALL, px, py)
        a.sample("ux", px[:1], py[:1])
        a.step(6)
        b.step(6)
        assert np.array_equal(a.populations(), b.populations())
    finally:
        a.close()
        b.close()


# ---- trajectories -------------------------------------------------------------------------------------

def seeds(nx, ny, n=130, seed=11):
    x, y = point_set(nx, ny, n, seed)
    return x, y


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_trajectory_at_stride_one(gpu, nx, ny, precision):
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        x0, y0 = seeds(nx, ny)
        A.set_tracers(x0, y0, stride=1)
        assert A.tracer_info() == {"n": 130, "stride": 1, "updates": 0}
        A.step(12)
        x, y, laps, path = host_trajectory(B, x0, y0, np.zeros(130, dtype=np.int32), 1, pieces(0, 1, 0, [12]))
        gx, gy, gl = A.tracers()
        assert np.median(path) > 0  # the tracers moved
        assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gl, laps)
        assert A.tracer_info()["updates"] == 12
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("stride,updates", [(5, 4), (7, 2), (8, 2)])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_trajectory_across_calls(gpu, nx, ny, precision, stride, updates):
    """step(3); step(4); step(13) with tracers set at t0 = 2: the updates fall inside the calls and count
    on across them (stride 5: after iterations 7, 12, 17, 22)."""
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        B.step(2)
        x0, y0 = seeds(nx, ny)
        A.set_tracers(x0, y0, stride=stride)
        calls = [3, 4, 13]
        plan = pieces(2, stride, 2, calls)
        assert sum(n for n, _ in plan) == 20 and sum(1 for _, u in plan if u) == updates
        assert max(n for n, _ in plan) <= stride
        for n in calls:
            A.step(n)
        x, y, laps, path = host_trajectory(B, x0, y0, np.zeros(130, dtype=np.int32), stride, plan)
        gx, gy, gl = A.tracers()
        assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gl, laps)
        assert A.tracer_info() == {"n": 130, "stride": stride, "updates": updates}
        assert A.steps == B.steps == 22
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


def fast_state(nx, ny):
    """|u| ~ 0.02: u_x > 0 in the upper half and < 0 in the lower half, u_y towards the nearer wall."""
    yy = np.repeat(np.arange(ny), nx).astype(float)
    upper = yy >= ny / 2
    rho = np.ones(nx * ny)
    ux = np.where(upper, 0.02, -0.02)
    uy = np.where(upper, 0.015, -0.015)
    return rho, np.concatenate([ux, uy])


def edge_seeds(nx, ny):
    """Tracers within one update of x = XDIM (upper half), of x = 0 (lower half) and of both walls."""
    up = np.arange(ny // 2 + 1, ny - 1, dtype=float)
    lo = np.arange(1, ny // 2 - 1, dtype=float)
    xs = np.arange(1, nx - 1, 3, dtype=float)
    x = np.concatenate([np.full(up.size, nx - 0.004), np.full(lo.size, 0.003), xs + 0.37, xs + 0.61,
                        [nx - 0.001, 0.001]])
    y = np.concatenate([up + 0.3, lo + 0.6, np.full(xs.size, ny - 1 - 0.002), np.full(xs.size, 0.0015),
                        [ny - 1 - 0.001, 0.001]])
    return x, y


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_wrap_and_clamp(gpu, nx, ny, precision):
    state = fast_state(nx, ny)
    A = new_lattice(gpu, nx, ny, precision, state=state)
    B = new_lattice(gpu, nx, ny, precision, state=state)
    try:
        x0, y0 = edge_seeds(nx, ny)
        n = x0.size
        A.set_tracers(x0, y0, stride=1)
        A.step(4)
        x, y, laps, _ = host_trajectory(B, x0, y0, np.zeros(n, dtype=np.int32), 1, pieces(0, 1, 0, [4]))
        # the case is not empty: in the reference itself a wrap each way and a clamp at each wall
        assert np.any(laps > 0) and np.any(laps < 0), laps
        assert np.any((y == 0.0) & (y0 > 0.0)) and np.any((y == ny - 1.0) & (y0 < ny - 1.0)), (y.min(), y.max())
        gx, gy, gl = A.tracers()
        assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gl, laps)
        assert np.all((gx >= 0) & (gx < nx) & (gy >= 0) & (gy <= ny - 1))
    finally:
        A.close()
        B.close()


def moving_points(nx, ny, steps):
    """The five points of test_gpu_fields.py moving a little every iteration: a schedule of `steps` entries."""
    s0, us0, eps0 = points(nx, ny)
    s = np.empty((steps, s0.size), dtype=np.float32)
    us = np.tile(us0, (steps, 1)).astype(np.float32)
    for it in range(steps):
        s[it] = s0
        s[it, 0::2] += np.float32(0.05) * np.sin(0.7 * it + np.arange(5)).astype(np.float32)
        s[it, 1::2] += np.float32(0.04) * np.cos(0.5 * it + np.arange(5)).astype(np.float32)
    s[:, 0::2] = np.clip(s[:, 0::2], 0.0, nx)
    return s, us, np.tile(eps0, (steps, 1)).astype(np.int32)


@pytest.mark.parametrize("stride", [1, 3, 6])
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_trajectory_with_moving_ib_points(gpu, nx, ny, stride):
    A = new_lattice(gpu, nx, ny, "f64", with_points=True)
    B = new_lattice(gpu, nx, ny, "f64", with_points=True)
    try:
        sched = moving_points(nx, ny, 12)
        A.set_lagrangian_steps(*sched)
        B.set_lagrangian_steps(*sched)
        x0, y0 = seeds(nx, ny)
        A.set_tracers(x0, y0, stride=stride)
        A.step(12)
        x, y, laps, path = host_trajectory(B, x0, y0, np.zeros(130, dtype=np.int32), stride, pieces(0, stride, 0, [12]))
        gx, gy, gl = A.tracers()
        bound = 1e-9 * (path + 1.0)
        ex, ey = np.abs(gx - x), np.abs(gy - y)
        print(f"{nx}x{ny} stride {stride}: max |dx| {ex.max():.3e} max |dy| {ey.max():.3e} min bound {bound.min():.3e}")
        assert np.array_equal(gl, laps)
        assert np.all(ex <= bound) and np.all(ey <= bound), (ex.max(), ey.max())
        assert A.tracer_info()["updates"] == 12 // stride
        # the IB force reached the tracers: the same run without points moves them elsewhere
        Cn = new_lattice(gpu, nx, ny, "f64")
        try:
            Cn.set_tracers(x0, y0, stride=stride)
            Cn.step(12)
            assert not np.array_equal(Cn.tracers()[0], gx)
        finally:
            Cn.close()
    finally:
        A.close()
        B.close()


# ---- lifecycle ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_removing_the_tracers_restores_the_old_path(gpu, precision):
    nx, ny = LATTICES[1]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        x0, y0 = seeds(nx, ny)
        A.set_tracers(x0, y0, stride=1)
        A.step(3)
        for _ in range(3):  # the pieces A's call was cut into
            B.step(1)
        A.set_tracers([], [])
        assert A.tracer_info()["n"] == 0 and A.tracers()[0].size == 0
        ta, tb = A.timing(), B.timing()
        A.step(14)
        B.step(14)
        ta1, tb1 = A.timing(), B.timing()
        for k in ("deep_launches", "deep_iterations"):
            assert ta1[k] - ta[k] == tb1[k] - tb[k], (k, ta[k], ta1[k], tb[k], tb1[k])
        assert tb1["deep_launches"] - tb["deep_launches"] > 0  # the path compared is the deep sweep
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


def test_set_state_keeps_and_a_checkpoint_drops_the_tracers(gpu, tmp_path):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        x0, y0 = seeds(nx, ny)
        A.set_tracers(x0, y0, stride=3)
        A.step(4)  # one update, one iteration into the next interval
        x, y, laps, _ = host_trajectory(B, x0, y0, np.zeros(130, dtype=np.int32), 3, pieces(0, 3, 0, [4]))
        # a new state: positions, laps and the count stay, the next update is `stride` iterations on
        rho, u = W.perturbed_state(nx, ny, 8)
        A.set_state(rho, u)
        B.set_state(rho, u)
        assert A.tracer_info() == {"n": 130, "stride": 3, "updates": 1}
        assert np.array_equal(A.tracers()[0], x)
        A.step(2)
        assert A.tracer_info()["updates"] == 1
        A.step(1)
        x, y, laps, _ = host_trajectory(B, x, y, laps, 3, [(2, False), (1, True)])
        gx, gy, gl = A.tracers()
        assert A.tracer_info()["updates"] == 2
        assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gl, laps)
        ck = str(tmp_path / "ck")
        A.save_checkpoint(ck)
        A.load_checkpoint(ck)
        assert A.tracer_info()["n"] == 0
        A.step(5)
        B.step(5)
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


def test_argument_errors_leave_the_context_and_its_tracers(gpu):
    nx, ny = LATTICES[0]
    lat = new_lattice(gpu, nx, ny, "f64", with_points=True)
    twin = new_lattice(gpu, nx, ny, "f64", with_points=True)
    try:
        lat.step(1)
        twin.step(1)
        x0, y0 = seeds(nx, ny, 5)
        lat.set_tracers(x0, y0, stride=2)
        lib, h = lat._lib, lat.handle
        good = np.array([1.5, 2.5, 3.5])
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        bad_positions = {
            "x = XDIM": (np.array([1.5, float(nx), 3.5]), good),
            "x < 0": (np.array([1.5, -1e-9, 3.5]), good),
            "y > YDIM-1": (good, np.array([1.5, np.nextafter(ny - 1.0, ny), 2.0])),
            "y < 0": (good, np.array([1.5, -0.5, 2.0])),
            "NaN x": (np.array([np.nan, 2.5, 3.5]), good),
            "inf y": (good, np.array([1.5, np.inf, 2.0])),
        }
        out = np.full(7 * 3, -7.0)
        for name, (bx, by) in bad_positions.items():
            assert lib.iblb_sample_points(h, 3, p(bx), p(by), 127, p(out)) == L.IBLB_ERR_ARG, name
            assert lib.iblb_set_tracers(h, 3, p(bx), p(by), 1) == L.IBLB_ERR_ARG, name
            assert lib.iblb_last_error(h), name
        assert lib.iblb_sample_points(h, -1, p(good), p(good), 1, p(out)) == L.IBLB_ERR_ARG
        assert lib.iblb_sample_points(h, 3, p(good), p(good), 0, p(out)) == L.IBLB_ERR_ARG
        assert lib.iblb_sample_points(h, 3, p(good), p(good), 128, p(out)) == L.IBLB_ERR_ARG
        assert lib.iblb_sample_points(h, 3, None, p(good), 1, p(out)) == L.IBLB_ERR_ARG
        assert lib.iblb_sample_points(h, 3, p(good), p(good), 1, None) == L.IBLB_ERR_ARG
        assert lib.iblb_sample_points(h, 0, None, None, 1, None) == L.IBLB_OK
        assert lib.iblb_set_tracers(h, -1, p(good), p(good), 1) == L.IBLB_ERR_ARG
        assert lib.iblb_set_tracers(h, 3, p(good), p(good), 0) == L.IBLB_ERR_ARG
        assert lib.iblb_set_tracers(h, 3, None, p(good), 1) == L.IBLB_ERR_ARG
        assert np.all(out == -7.0)
        with pytest.raises(ValueError):
            lat.sample(["pressure"], good, good)
        # the previous tracers are as they were, and the context still runs and updates them
        assert lat.tracer_info() == {"n": 5, "stride": 2, "updates": 0}
        gx, gy, gl = lat.tracers()
        assert np.array_equal(gx, x0) and np.array_equal(gy, y0) and not gl.any()
        lat.step(2)
        twin.step(2)
        f = twin.fields(["ux", "uy"])
        x, y, laps = T.advect(f["ux"], f["uy"], x0, y0, gl, 2)
        gx, gy, gl = lat.tracers()
        assert lat.tracer_info()["updates"] == 1
        assert np.max(np.abs(gx - x)) <= 1e-9 and np.max(np.abs(gy - y)) <= 1e-9 and np.array_equal(gl, laps)
        assert not np.array_equal(gx, x0)
    finally:
        lat.close()
        twin.close()


def test_a_slab_of_a_group_is_refused(gpu):
    nx, ny = LATTICES[0]
    rho, u = W.perturbed_state(nx, ny, 7)
    slabs = []
    for xb, xc in gpu.plan_slabs(nx, 2):
        s = gpu.Lattice(nx, ny, W.TAU, W.TAU2, body_force=BODY_FORCE, x_begin=xb, x_count=xc)
        s.set_state(gpu.split_state(rho, 1, nx, ny, xb, xc), gpu.split_state(u, 2, nx, ny, xb, xc))
        slabs.append(s)
    try:
        group = gpu.LocalGroup(slabs)
        group.step(2)
        for s in slabs:
            x, y = np.array([s.x_begin + 1.5]), np.array([2.5])
            for call in (lambda: s.sample("ux", x, y), lambda: s.set_tracers(x, y, 1)):
                with pytest.raises(gpu.IblbError) as e:
                    call()
                assert e.value.code == L.IBLB_ERR_UNSUPPORTED
                msg = s._lib.iblb_last_error(s.handle)
                assert msg and len(msg.decode()) > 0
            assert s.tracer_info()["n"] == 0
    finally:
        for s in slabs:
            s.close()
