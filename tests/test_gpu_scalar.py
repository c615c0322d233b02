"""The passive scalar of iblb_set_scalar on the GPU against tests/scalar_ref.py (checked on the CPU by
tests/test_scalar_ref.py) applied to what Lattice.fields returns for a twin lattice stepped in the pieces iblb_step
cuts its calls into.

Lattices 20 x 18, 37 x 23 (an odd size, fewer rows than a wave) and 16 x 300 (more rows than a 256-lane workgroup,
not a multiple of 64), f64 and f32 storage, tau 0.8, a seeded perturbed state and a body force with both components
(as tests/test_gpu_average.py).

Every comparison is `==` (np.array_equal): the device takes the velocity from the functions iblb_get_fields uses and
does every operation of the rule once, rounded once, which is what the numpy twin does.  The twin lattices carry no IB
points: the spread's atomic order may differ in the last bits between two contexts (tests/test_gpu_tracers.py).  With
moving IB points the reference therefore takes the same lattice's own fields, read after calls that end on an event.
The driver's scenario has cilia and is a second process: its rows are compared at 1e-9 * (1 + |C|), the bound of
tests/test_app_tracers.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

import app_model as M
import average_ref as AR
import scalar_ref as S
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_app import ARGS, read, run_app
from test_gpu_average import ALL, assert_bins_equal, twin_samples, windows
from test_gpu_fields import BODY_FORCE
from test_gpu_tracers import host_trajectory, moving_points, new_lattice, seeds

pytestmark = pytest.mark.gpu

LATTICES = [(20, 18), (37, 23), (16, 300)]
PRECISIONS = ["f64", "f32"]
TAU = 0.8
WALLS = {"no flux": S.NO_FLUX_WALLS, "value below": ((S.VALUE, 0.25), (S.NOFLUX, 0.0))}

_C0 = {}


def seeded_c0(nx, ny):
    """A seeded concentration in [0, 1) with a step across the channel's middle (computed once per size)."""
    if (nx, ny) not in _C0:
        c = np.random.default_rng(nx * 1000 + ny).uniform(0.0, 0.5, (ny, nx))
        c[: ny // 2] += 0.5
        c.setflags(write=False)
        _C0[(nx, ny)] = c
    return _C0[(nx, ny)]


def velocity(lat):
    f = lat.fields(["ux", "uy"])
    return f["ux"], f["uy"]


def host_scalar(B, g, plan, stride, walls=S.NO_FLUX_WALLS, key="scalar"):
    """Step the twin B in the pieces of `plan` and run the scalar's events on the host."""
    for n, due in plan:
        B.step(n)
        if due[key]:
            g = S.event(g, *velocity(B), TAU, stride, walls)
    return g


def assert_scalar_equal(A, g, what):
    got = A.scalar_populations()
    assert got.shape == g.shape, what
    assert np.array_equal(got, g), (what, np.max(np.abs(got - g)))
    assert np.array_equal(A.scalar(), S.concentration(g)), what


# ---- 1. the scalar equals the twin -----------------------------------------------------------------------

@pytest.mark.parametrize("walls", list(WALLS))
@pytest.mark.parametrize("stride", [1, 5, 7, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_equals_the_twin(gpu, nx, ny, precision, stride, walls):
    """step(3); step(4); step(13) with the scalar set at t0 = 2: the events fall inside the calls and count on
    across them."""
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        B.step(2)
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=stride, walls=WALLS[walls])
        info = A.scalar_info()
        assert (info["tau"], info["stride"], info["updates"]) == (TAU, stride, 0)
        assert info["walls"] == tuple((k, float(v)) for k, v in WALLS[walls])
        g = S.equilibrium(c0, *velocity(B))
        assert_scalar_equal(A, g, "at the set")
        calls = [3, 4, 13]
        plan = S.pieces(calls, 2, scalar=(2, stride))
        assert sum(n for n, _ in plan) == 20 and max(n for n, _ in plan) <= stride
        for n in calls:
            A.step(n)
        g = host_scalar(B, g, plan, stride, WALLS[walls])
        assert_scalar_equal(A, g, "after 20 iterations")
        assert A.scalar_info()["updates"] == 20 // stride == sum(1 for _, d in plan if d["scalar"])
        assert A.steps == B.steps == 22
        assert np.array_equal(A.populations(), B.populations())
        # the case is not empty: C changed, and the velocity entered it
        assert np.any(A.scalar() != c0)
        zero = np.zeros((ny, nx))
        still = S.event(S.equilibrium(c0, zero, zero), zero, zero, TAU, stride * (20 // stride), WALLS[walls])
        assert not np.array_equal(S.concentration(still), A.scalar())
    finally:
        A.close()
        B.close()


# ---- 2. with moving IB points ----------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 3, 6])
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_with_moving_ib_points(gpu, nx, ny, stride):
    """Every call ends on an event, and the reference takes the lattice's own velocity read after the call: the
    owed IB force is in it, bit for bit."""
    A = new_lattice(gpu, nx, ny, "f64", with_points=True)
    Cn = new_lattice(gpu, nx, ny, "f64")
    try:
        A.set_lagrangian_steps(*moving_points(nx, ny, 12))
        c0 = seeded_c0(nx, ny)
        g = S.equilibrium(c0, *velocity(A))
        for lat in (A, Cn):
            lat.set_scalar(c0, tau=TAU, stride=stride)
        for _ in range(12 // stride):
            A.step(stride)
            g = S.event(g, *velocity(A), TAU, stride)
            assert_scalar_equal(A, g, f"after iteration {A.steps}")
        assert A.scalar_info()["updates"] == 12 // stride
        # the IB force reached the scalar: the same run without points gives another field
        Cn.step(12)
        assert not np.array_equal(Cn.scalar(), A.scalar())
    finally:
        A.close()
        Cn.close()


# ---- 3. all three observers ------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES[:2])
def test_with_tracers_and_averages(gpu, nx, ny, precision):
    """The scalar every 5, tracers every 3 and samples every 4 iterations over step(9); step(11): the calls are cut
    at the union of the three event sets, and each observer equals its own reference."""
    A = new_lattice(gpu, nx, ny, precision)
    Bs, Bt, Ba = (new_lattice(gpu, nx, ny, precision) for _ in range(3))
    try:
        x0, y0 = seeds(nx, ny)
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=5)
        A.set_tracers(x0, y0, stride=3)
        A.set_average(ALL, stride=4, nbins=2, squares=True, uxuy=True)
        calls = [9, 11]
        for n in calls:
            A.step(n)
        plan = S.pieces(calls, 0, scalar=(0, 5), tracers=(0, 3), average=(0, 4))
        assert [sum(1 for _, d in plan if d[k]) for k in ("scalar", "tracers", "average")] == [4, 6, 5]
        assert any(d["scalar"] and d["average"] for _, d in plan) and any(d["tracers"] and d["scalar"] for _, d in plan)
        g = host_scalar(Bs, S.equilibrium(c0, *velocity(Bs)), plan, 5)
        assert_scalar_equal(A, g, "with tracers and averages")
        x, y, laps, path = host_trajectory(Bt, x0, y0, np.zeros(x0.size, dtype=np.int32), 3,
                                           [(n, d["tracers"]) for n, d in plan])
        gx, gy, gl = A.tracers()
        assert np.median(path) > 0
        assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gl, laps)
        samples = twin_samples(Ba, [(n, d["tracers"], d["average"]) for n, d in plan])
        assert_bins_equal(A, AR.accumulate(samples, 2, squares=True, uxuy=True), "with the scalar")
        assert (A.scalar_info()["updates"], A.tracer_info()["updates"], A.average_info()["samples_total"]) == (4, 6, 5)
        assert np.array_equal(A.populations(), Bs.populations())
    finally:
        for lat in (A, Bs, Bt, Ba):
            lat.close()


# ---- 4. windows ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_windows(gpu, nx, ny, precision):
    A = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=2)
        A.step(4)
        whole = A.scalar()
        assert whole.shape == (ny, nx) and np.any(whole != seeded_c0(nx, ny))
        for name, w in windows(nx, ny).items():
            if w is None:
                continue
            x0, y0, wnx, wny, sx, sy = w
            got = A.scalar(w)
            assert got.shape == (wny, wnx), name
            assert np.array_equal(got, whole[y0:y0 + (wny - 1) * sy + 1:sy, x0:x0 + (wnx - 1) * sx + 1:sx]), name
    finally:
        A.close()


# ---- 5. lifecycle ----------------------------------------------------------------------------------------

def test_set_state_keeps_and_a_checkpoint_drops_the_scalar(gpu, tmp_path):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=3)
        g = S.equilibrium(c0, *velocity(B))
        A.step(4)  # one event, one iteration into the next interval
        g = host_scalar(B, g, S.pieces([4], 0, scalar=(0, 3)), 3)
        assert_scalar_equal(A, g, "before the new state")
        # a new state: populations and the count stay, the next event is `stride` iterations on
        rho, u = W.perturbed_state(nx, ny, 8)
        A.set_state(rho, u)
        B.set_state(rho, u)
        assert A.scalar_info()["updates"] == 1
        assert_scalar_equal(A, g, "after set_state")
        A.step(2)
        assert A.scalar_info()["updates"] == 1
        assert_scalar_equal(A, g, "two iterations into the new state")
        A.step(1)
        g = host_scalar(B, g, [(2, {"scalar": False}), (1, {"scalar": True})], 3)
        assert A.scalar_info()["updates"] == 2
        assert_scalar_equal(A, g, "the first event of the new state")
        # a checkpoint holds no scalar
        ck = str(tmp_path / "ck")
        A.save_checkpoint(ck)
        A.load_checkpoint(ck)
        assert A.scalar_info()["stride"] == 0 and A.scalar_info()["updates"] == 0
        with pytest.raises(gpu.IblbError) as e:
            A.scalar()
        assert e.value.code == L.IBLB_ERR_STATE
        A.step(5)
        B.step(5)
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_removing_the_scalar_restores_the_old_path(gpu, precision):
    nx, ny = LATTICES[1]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=1)
        A.step(3)
        for _ in range(3):  # the pieces A's call was cut into
            B.step(1)
        A.remove_scalar()
        assert A.scalar_info() == {"tau": 0.0, "stride": 0, "walls": ((0, 0.0), (0, 0.0)), "updates": 0}
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


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_stride_of_seven_keeps_the_deep_sweep(gpu, precision):
    nx, ny = LATTICES[1]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(7)
        B.step(7)
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=7)
        ta, tb = A.timing(), B.timing()
        A.step(14)
        B.step(7)
        B.step(7)
        ta1, tb1 = A.timing(), B.timing()
        for k in ("deep_launches", "deep_iterations"):
            assert ta1[k] - ta[k] == tb1[k] - tb[k], (k, ta[k], ta1[k], tb[k], tb1[k])
        assert tb1["deep_launches"] - tb["deep_launches"] > 0
        assert A.scalar_info()["updates"] == 2
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 6. restart ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("walls", list(WALLS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_restart_from_the_populations(gpu, precision, walls):
    """scalar_populations() at an event iteration, set_scalar(g0=...) on another context at the same state, then
    both continue: the restarted run equals the uninterrupted one."""
    nx, ny = LATTICES[1]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=4, walls=WALLS[walls])
        A.step(8)
        B.step(8)
        saved = A.scalar_populations()
        B.set_scalar(g0=saved, tau=TAU, stride=4, walls=WALLS[walls])
        assert np.array_equal(B.scalar_populations(), saved) and B.scalar_info()["updates"] == 0
        A.step(9)
        B.step(9)
        assert (A.scalar_info()["updates"], B.scalar_info()["updates"]) == (4, 2)
        assert np.array_equal(A.scalar_populations(), B.scalar_populations())
        assert np.array_equal(A.scalar(), B.scalar()) and not np.array_equal(A.scalar_populations(), saved)
    finally:
        A.close()
        B.close()


# ---- 7. refusals leave everything as it was ----------------------------------------------------------------

def test_argument_errors_leave_the_scalar_as_it_was(gpu):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        lib, h = A._lib, A.handle
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        out = np.full(5 * nx * ny, -7.0)
        # no scalar set: the getters are refused, nothing written
        assert lib.iblb_get_scalar(h, None, p(out)) == L.IBLB_ERR_STATE
        assert lib.iblb_get_scalar_populations(h, p(out)) == L.IBLB_ERR_STATE
        assert np.all(out == -7.0) and lib.iblb_last_error(h)

        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=3, walls=WALLS["value below"])
        g = S.equilibrium(c0, *velocity(B))
        A.step(4)
        g = host_scalar(B, g, S.pieces([4], 0, scalar=(0, 3)), 3, WALLS["value below"])
        info = A.scalar_info()
        cfg = lambda tau=0.9, stride=2, kinds=(0, 0), values=(0.0, 0.0): L.Scalar(
            tau, stride, (C.c_int * 2)(*kinds), (C.c_double * 2)(*values))
        c1, g1 = np.ones(nx * ny), np.ones(5 * nx * ny)
        bad_sets = {
            "tau 0.5": (cfg(tau=0.5), c1, None),
            "tau NaN": (cfg(tau=float("nan")), c1, None),
            "tau inf": (cfg(tau=float("inf")), c1, None),
            "stride 0": (cfg(stride=0), c1, None),
            "a wall kind of 2": (cfg(kinds=(0, 2)), c1, None),
            "a wall kind of -1": (cfg(kinds=(-1, 0)), c1, None),
            "a NaN wall value under _VALUE": (cfg(kinds=(1, 0), values=(float("nan"), 0.0)), c1, None),
            "an infinite wall value under _VALUE": (cfg(kinds=(0, 1), values=(0.0, float("inf"))), c1, None),
            "both c0 and g0": (cfg(), c1, g1),
            "neither c0 nor g0": (cfg(), None, None),
        }
        for name, (k, a, b) in bad_sets.items():
            rc = lib.iblb_set_scalar(h, C.byref(k), None if a is None else p(a), None if b is None else p(b))
            assert rc == L.IBLB_ERR_ARG, name
            assert lib.iblb_last_error(h), name
            assert A.scalar_info() == info, name
        # a NaN wall value is fine where the wall is no-flux
        ok = cfg(kinds=(0, 0), values=(float("nan"), float("nan")))
        T = new_lattice(gpu, nx, ny, "f64")
        try:
            assert T._lib.iblb_set_scalar(T.handle, C.byref(ok), p(c1), None) == L.IBLB_OK
        finally:
            T.close()
        bad_windows = {
            "past the last column": L.Window(nx - 2, 0, 2, 2, 2, 1),
            "past the last row": L.Window(0, 0, 2, ny + 1, 1, 1),
            "no samples": L.Window(0, 0, 0, 2, 1, 1),
            "stride 0": L.Window(0, 0, 2, 2, 0, 1),
        }
        for name, w in bad_windows.items():
            assert lib.iblb_get_scalar(h, C.byref(w), p(out)) == L.IBLB_ERR_ARG, name
        assert lib.iblb_get_scalar(h, None, None) == L.IBLB_ERR_ARG
        assert lib.iblb_get_scalar_populations(h, None) == L.IBLB_ERR_ARG
        assert np.all(out == -7.0)
        # the scalar is as it was, and its next event (after iteration 6) still matches the twin
        assert A.scalar_info() == info
        assert_scalar_equal(A, g, "after the refused calls")
        A.step(1)
        assert A.scalar_info()["updates"] == 1
        A.step(1)
        g = host_scalar(B, g, [(2, {"scalar": True})], 3, WALLS["value below"])
        assert A.scalar_info()["updates"] == 2
        assert_scalar_equal(A, g, "the next event")
    finally:
        A.close()
        B.close()


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
            with pytest.raises(gpu.IblbError) as e:
                s.set_scalar(np.ones((ny, s.x_count)), tau=TAU, stride=2)
            assert e.value.code == L.IBLB_ERR_UNSUPPORTED
            msg = s._lib.iblb_last_error(s.handle)
            assert msg and len(msg.decode()) > 0
            assert s.scalar_info()["stride"] == 0
        group.step(2)
    finally:
        for s in slabs:
            s.close()


# ---- 8. the driver -----------------------------------------------------------------------------------------

SCALAR = (0.8, 2, 4, 2)  # tau, stride, sx, sy


def test_app_writes_the_scalar(gpu, tmp_path):
    p = M.params(ARGS)
    X, Y = p["XDIM"], M.YDIM
    tau, stride, sx, sy = SCALAR
    r = run_app(ARGS, tmp_path, IBLB_SCALAR=",".join(str(v) for v in SCALAR))
    assert r.returncode == 0, r.stdout + r.stderr

    wnx, wny = (X - 1) // sx + 1, (Y - 1) // sy + 1
    c0 = np.zeros((Y, X))
    c0[: Y // 2] = 1.0
    lat = gpu.Lattice(X, Y, p["TAU"], p["TAU2"], max_points=M.LENGTH * p["c_num"])
    try:
        lat.set_state()
        lat.set_cilia(p["c_num"], float(p["c_space"]), p["T"], p["p_step"])
        lat.set_scalar(c0, tau=tau, stride=stride)
        done, files = 0, 0
        ii, jj = np.meshgrid(np.arange(wnx) * sx, np.arange(wny) * sy)
        for it in range(0, p["ITERATIONS"], p["INTERVAL"]):
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            rows = [ln.split("\t") for ln in read(tmp_path, M.paths(p)["raw"] + f"{it}-scalar.dat").split("\n") if ln]
            assert len(rows) == wnx * wny and all(len(g) == 3 for g in rows)
            col = lambda k, conv=float: np.array([conv(g[k]) for g in rows]).reshape(wny, wnx)
            assert np.array_equal(col(0, int), ii) and np.array_equal(col(1, int), jj)
            want = lat.scalar((0, 0, wnx, wny, sx, sy))
            assert lat.scalar_info()["updates"] == done // stride
            if done < stride:  # no event yet: the seed's equilibrium at rest, bit for bit (%.17g round-trips a double)
                zero = np.zeros((Y, X))
                assert np.array_equal(col(2), S.concentration(S.equilibrium(c0, zero, zero))[::sy, ::sx])
            err = np.abs(col(2) - want)
            print(f"it {it}: max |dC| {err.max():.3e}")
            assert np.all(err <= 1e-9 * (1.0 + np.abs(want))), it
            files += 1
        assert files > 1 and np.any(lat.scalar() != c0)  # the scalar moved
    finally:
        lat.close()


def test_app_without_the_variable_writes_no_scalar_file(gpu, tmp_path):
    p = M.params(ARGS)
    r = run_app(ARGS, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    names = os.listdir(str(tmp_path) + "/" + M.paths(p)["raw"])
    assert "0-fluid.dat" in names and not [n for n in names if n.endswith("-scalar.dat")], names
