"""The scalar's source of iblb_set_scalar_source on the GPU against tests/scalar_source_ref.py (checked on the CPU by
tests/test_scalar_source_ref.py) applied to what Lattice.fields returns for a twin lattice stepped in the pieces
iblb_step cuts its calls into.

The lattices, precisions, state and helpers are those of tests/test_gpu_scalar.py: 20 x 18, 37 x 23 (odd, fewer rows
than a wave) and 16 x 300 (the top-wall lanes sit in the second workgroup), f64 and f32 storage, tau 0.8.  Every
population comparison is `==` (np.array_equal): the device does every operation of the rule once, rounded once, and
skips no term, which is what the numpy twin does.
"""
import ctypes as C

import numpy as np
import pytest

import average_ref as AR
import scalar_fields_ref as F
import scalar_ref as S
import scalar_source_ref as Q
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_fields import BODY_FORCE
from test_gpu_average import assert_bins_equal
from test_gpu_scalar import LATTICES, PRECISIONS, TAU, WALLS, assert_scalar_equal, seeded_c0, velocity
from test_gpu_tracers import moving_points, new_lattice

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
VALUE_BELOW = WALLS["value below"]
_SRC = {}


def sources(nx, ny):
    """{name: (Source, walls)} for one size, computed once: the four sources of the first test."""
    if (nx, ny) not in _SRC:
        rng = np.random.default_rng(nx * 977 + ny)
        field = rng.uniform(-2e-3, 4e-3, (ny, nx))
        f0, f1 = rng.uniform(-3e-3, 3e-3, (2, nx))
        v0 = 0.25 + 0.2 * np.sin(2.0 * np.pi * np.arange(nx) / nx)
        for a in (field, f0, f1, v0):
            a.setflags(write=False)
        assert np.any(f0 < 0) and np.any(f0 > 0) and np.any(f1 < 0) and np.any(f1 > 0)
        _SRC[(nx, ny)] = {
            "field and decay": (Q.Source(field, 0.02), S.NO_FLUX_WALLS),
            "wall flux": (Q.Source(None, 0.0, (f0, f1)), S.NO_FLUX_WALLS),
            "value profile below, flux above": (Q.Source(field, 0.02, (None, f1), (v0, None)), VALUE_BELOW),
            "nothing": (Q.Source(), S.NO_FLUX_WALLS),
            "budget": (Q.Source(field, 0.02, (f0, f1)), S.NO_FLUX_WALLS),
        }
    return _SRC[(nx, ny)]


def host_run(B, g, plan, stride, src, walls=S.NO_FLUX_WALLS):
    """Step the twin B in the pieces of `plan` and run the scalar's events with the source on the host."""
    for n, due in plan:
        B.step(n)
        if due["scalar"]:
            g = Q.event(g, *velocity(B), TAU, stride, src, walls)
    return g


def assert_source_equal(A, g, src, walls, what):
    assert_scalar_equal(A, g, what)
    if src is not None:
        for got, want in zip(A.scalar_wall_flux(), Q.wall_flux(g, src, walls)):
            assert np.array_equal(got, want), (what, "wall flux")


def code_of(gpu, call):
    with pytest.raises(gpu.IblbError) as e:
        call()
    return e.value.code


# ---- 1. the scalar with a source equals the twin -------------------------------------------------------------

@pytest.mark.parametrize("name", ["field and decay", "wall flux", "value profile below, flux above", "nothing"])
@pytest.mark.parametrize("stride", [1, 5, 7])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_equals_the_twin(gpu, nx, ny, precision, stride, name):
    """step(9); step(11) with the scalar and its source set at t0 = 2: the events fall inside the calls and count on
    across them."""
    src, walls = sources(nx, ny)[name]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        B.step(2)
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=stride, walls=walls)
        A.set_scalar_source(**src.kwargs())
        assert A.scalar_source_info() == {"decay": src.decay, "present": src.present()}
        assert A.scalar_info()["updates"] == 0
        g = S.equilibrium(c0, *velocity(B))
        assert_scalar_equal(A, g, "at the set")
        t = 2
        for n in (9, 11):
            plan = S.pieces([n], t, scalar=(2, stride))
            assert any(d["scalar"] for _, d in plan)
            A.step(n)
            g = host_run(B, g, plan, stride, src, walls)
            t += n
            assert_source_equal(A, g, src, walls, f"after iteration {t}")
        assert A.scalar_info()["updates"] == 20 // stride
        assert A.steps == B.steps == 22
        assert np.array_equal(A.populations(), B.populations())
        # the case is not empty: the source entered C, unless it holds nothing
        plain = new_lattice(gpu, nx, ny, precision)
        try:
            plain.step(2)
            plain.set_scalar(c0, tau=TAU, stride=stride, walls=walls)
            plain.step(9)
            plain.step(11)
            assert np.array_equal(plain.scalar_populations(), A.scalar_populations()) == (name == "nothing")
        finally:
            plain.close()
    finally:
        A.close()
        B.close()


# ---- 2. set and removed in mid-run ---------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_set_and_removed_between_events(gpu, precision):
    """Stride 7.  An event without a source after iteration 7, the source set after iteration 10, events with it after
    14 and 21, removed, events of the old rule after 28 and 35.  The twin is stepped in the same pieces: the deep
    launches are as many."""
    nx, ny = LATTICES[1]
    src, walls = sources(nx, ny)["value profile below, flux above"]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=7, walls=walls)
        g = plain = S.equilibrium(c0, *velocity(B))  # plain: the same run under the rule without a source
        ta, tb = A.timing(), B.timing()
        t = 0
        for n, s in ((10, None), (11, src), (14, None)):
            A.step(n)
            for m, due in S.pieces([n], t, scalar=(0, 7)):
                B.step(m)
                if due["scalar"]:
                    uv = velocity(B)
                    g = Q.event(g, *uv, TAU, 7, s, walls)
                    plain = S.event(plain, *uv, TAU, 7, walls)
            t += n
            assert_source_equal(A, g, s, walls, f"after iteration {t}")
            if t == 10:
                assert np.array_equal(g, plain)
                A.set_scalar_source(**src.kwargs())
                assert A.scalar_info()["updates"] == 1  # the set moves neither t0 nor the count
                assert_scalar_equal(A, g, "at the set of the source")
            elif t == 21:
                assert not np.array_equal(g, plain)
                A.remove_scalar_source()
                assert A.scalar_source_info() == {"decay": 0.0, "present": 0}
        assert A.scalar_info()["updates"] == 5
        ta1, tb1 = A.timing(), B.timing()
        assert ta1["deep_launches"] - ta["deep_launches"] == tb1["deep_launches"] - tb["deep_launches"] > 0
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 3. with moving IB points --------------------------------------------------------------------------------

def test_with_moving_ib_points(gpu):
    """Every call ends on an event, and the reference takes the lattice's own velocity read after the call."""
    nx, ny = LATTICES[1]
    stride = 3
    src, walls = sources(nx, ny)["budget"]
    A = new_lattice(gpu, nx, ny, "f64", with_points=True)
    try:
        A.set_lagrangian_steps(*moving_points(nx, ny, 12))
        c0 = seeded_c0(nx, ny)
        g = S.equilibrium(c0, *velocity(A))
        A.set_scalar(c0, tau=TAU, stride=stride)
        A.set_scalar_source(**src.kwargs())
        for _ in range(12 // stride):
            A.step(stride)
            g = Q.event(g, *velocity(A), TAU, stride, src, walls)
            assert_source_equal(A, g, src, walls, f"after iteration {A.steps}")
        assert A.scalar_info()["updates"] == 12 // stride
    finally:
        A.close()


# ---- 4. with an average of the scalar ------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_average_samples_c_after_the_event_with_its_source(gpu, precision):
    nx, ny = LATTICES[1]
    src, walls = sources(nx, ny)["value profile below, flux above"]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=5, walls=walls)
        A.set_scalar_source(**src.kwargs())
        A.set_average(["c", "cux"], stride=5, nbins=2)
        g = S.equilibrium(c0, *velocity(B))
        calls = [9, 11]
        for n in calls:
            A.step(n)
        samples = []
        for n, due in S.pieces(calls, 0, scalar=(0, 5)):
            B.step(n)
            if due["scalar"]:
                ux, uy = velocity(B)
                g = Q.event(g, ux, uy, TAU, 5, src, walls)
                f = F.scalar_fields(g, ux, uy)
                samples.append({"c": f["c"], "cux": f["cux"]})
        assert len(samples) == 4
        assert_bins_equal(A, AR.accumulate(samples, 2), "with a source")
        assert_source_equal(A, g, src, walls, "under the average")
    finally:
        A.close()
        B.close()


# ---- 5. the budget on the device -----------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", LATTICES)
def test_budget_on_the_device(gpu, nx, ny):
    """Stride 1 between no-flux walls: sum(C) of reduce(["c"]) changes over one event by sum(r) + sum(wall_flux), both
    from the C read before the event, within the bound of the CPU check scaled by the cell count over 35."""
    src, walls = sources(nx, ny)["budget"]
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=1)
        A.set_scalar_source(**src.kwargs())
        A.step(3)
        C0 = A.scalar()
        s0 = A.reduce(["c"])["c"].sum
        A.step(1)
        C1 = A.scalar()
        s1 = A.reduce(["c"])["c"].sum
        want = np.sum(Q.rate(C0, src)) + np.sum(src.wall_flux[0] + src.wall_flux[1])
        bound = 64 * EPS * (np.sum(np.abs(C0)) + np.sum(np.abs(C1))) * (nx * ny / 35.0)
        print(f"{nx} x {ny}: d sum(C) {s1 - s0:.6e}, want {want:.6e}, |diff| {abs(s1 - s0 - want):.3e}, bound {bound:.3e}")
        assert want != 0.0 and abs((s1 - s0) - want) <= bound
    finally:
        A.close()


# ---- 6. round trip and info ----------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", LATTICES)
def test_round_trip_and_info(gpu, nx, ny):
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        assert A.scalar_source_info() == {"decay": 0.0, "present": 0}
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=2, walls=VALUE_BELOW)
        assert A.scalar_source_info() == {"decay": 0.0, "present": 0}
        assert code_of(gpu, A.scalar_source) == L.IBLB_ERR_STATE
        src, _ = sources(nx, ny)["value profile below, flux above"]
        A.set_scalar_source(**src.kwargs())
        got = A.scalar_source()
        assert got.shape == (ny, nx) and np.array_equal(got, src.source)
        assert A.scalar_source_info() == {"decay": 0.02, "present": 1 | 2 | 8 | 16}
        # walls alone: the field reads as zeros
        A.set_scalar_source(wall_flux=(None, src.wall_flux[1]))
        assert np.array_equal(A.scalar_source(), np.zeros((ny, nx)))
        assert A.scalar_source_info() == {"decay": 0.0, "present": 1 | 8}
        A.set_scalar_source(decay=0.5)
        assert A.scalar_source_info() == {"decay": 0.5, "present": 1}
        # shape errors are raised before the call
        with pytest.raises(ValueError):
            A.set_scalar_source(source=np.zeros(nx * ny + 1))
        with pytest.raises(ValueError):
            A.set_scalar_source(wall_flux=(None, np.zeros(nx - 1)))
        with pytest.raises(ValueError):
            A.set_scalar_source(wall_value=(np.zeros(nx + 1), None))
        assert A.scalar_source_info() == {"decay": 0.5, "present": 1}
        A.remove_scalar_source()
        assert A.scalar_source_info() == {"decay": 0.0, "present": 0}
    finally:
        A.close()


# ---- 7. lifecycle --------------------------------------------------------------------------------------------

def test_set_state_keeps_and_a_new_scalar_or_a_checkpoint_drops_the_source(gpu, tmp_path):
    nx, ny = LATTICES[0]
    src, walls = sources(nx, ny)["value profile below, flux above"]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        A.set_scalar_source(**src.kwargs())
        info = A.scalar_source_info()
        g = S.equilibrium(c0, *velocity(B))
        A.step(4)
        g = host_run(B, g, S.pieces([4], 0, scalar=(0, 3)), 3, src, walls)
        assert_source_equal(A, g, src, walls, "before the new state")
        rho, u = W.perturbed_state(nx, ny, 8)
        A.set_state(rho, u)
        B.set_state(rho, u)
        assert A.scalar_source_info() == info and np.array_equal(A.scalar_source(), src.source)
        A.step(3)
        g = host_run(B, g, S.pieces([3], 0, scalar=(0, 3)), 3, src, walls)  # the plan restarts from 0
        assert A.scalar_info()["updates"] == 2
        assert_source_equal(A, g, src, walls, "the first event of the new state")
        # a replacement of the scalar drops the source, and so does its removal
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        assert A.scalar_source_info() == {"decay": 0.0, "present": 0}
        g = S.equilibrium(c0, *velocity(B))
        A.step(3)
        B.step(3)
        assert_scalar_equal(A, S.event(g, *velocity(B), TAU, 3, walls), "the old rule after the replacement")
        A.set_scalar_source(**src.kwargs())
        assert A.scalar_source_info() == info
        A.remove_scalar()
        assert A.scalar_source_info() == {"decay": 0.0, "present": 0}
        assert code_of(gpu, lambda: A.set_scalar_source(decay=0.1)) == L.IBLB_ERR_STATE
        # a checkpoint holds neither
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        A.set_scalar_source(**src.kwargs())
        ck = str(tmp_path / "ck")
        A.save_checkpoint(ck)
        A.load_checkpoint(ck)
        assert A.scalar_source_info() == {"decay": 0.0, "present": 0} and A.scalar_info()["stride"] == 0
        A.step(5)
        B.step(5)
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 8. refusals leave everything as it was ------------------------------------------------------------------

def test_errors_leave_the_source_as_it_was(gpu):
    nx, ny = LATTICES[0]
    src, walls = sources(nx, ny)["value profile below, flux above"]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    T = new_lattice(gpu, nx, ny, "f64")
    try:
        # no scalar
        assert code_of(gpu, lambda: A.set_scalar_source(decay=0.1)) == L.IBLB_ERR_STATE
        assert A._lib.iblb_last_error(A.handle)
        assert code_of(gpu, A.remove_scalar_source) == L.IBLB_ERR_STATE
        assert A.scalar_source_info() == {"decay": 0.0, "present": 0}

        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        A.set_scalar_source(**src.kwargs())
        g = S.equilibrium(c0, *velocity(B))
        A.step(4)
        g = host_run(B, g, S.pieces([4], 0, scalar=(0, 3)), 3, src, walls)
        info = A.scalar_source_info()
        nan = lambda n, shape=None: np.where(np.arange(n) == n // 2, np.nan, 0.1).reshape(shape or n)
        ok = np.full(nx, 0.1)
        bad = {
            "a negative decay": dict(decay=-1e-300),
            "a NaN decay": dict(decay=float("nan")),
            "an infinite decay": dict(decay=float("inf")),
            "a NaN in source": dict(source=nan(nx * ny, (ny, nx))),
            "an infinity in source": dict(source=np.where(np.arange(nx * ny) == nx * ny - 1, np.inf, 0.0)),
            "a NaN in wall_flux[1]": dict(wall_flux=(None, nan(nx))),
            "a NaN in wall_value[0]": dict(wall_value=(nan(nx), None)),
            "wall_flux on a _VALUE wall": dict(wall_flux=(ok, None)),
            "wall_value on a _NOFLUX wall": dict(wall_value=(None, ok)),
        }
        for name, kw in bad.items():
            assert code_of(gpu, lambda: A.set_scalar_source(**kw)) == L.IBLB_ERR_ARG, name
            assert A._lib.iblb_last_error(A.handle), name
            assert A.scalar_source_info() == info, name
        assert A._lib.iblb_get_scalar_source(A.handle, None) == L.IBLB_ERR_ARG
        assert A.scalar_source_info() == info
        # the other two arrays, on a scalar whose walls take them
        T.set_scalar(c0, tau=TAU, stride=3, walls=(VALUE_BELOW[1], VALUE_BELOW[0]))
        T.set_scalar_source(decay=0.25, wall_flux=(ok, None), wall_value=(None, ok))
        tinfo = T.scalar_source_info()
        assert tinfo == {"decay": 0.25, "present": 1 | 4 | 32}
        for name, kw in {"a NaN in wall_flux[0]": dict(wall_flux=(nan(nx), None)),
                         "a NaN in wall_value[1]": dict(wall_value=(None, nan(nx)))}.items():
            assert code_of(gpu, lambda: T.set_scalar_source(**kw)) == L.IBLB_ERR_ARG, name
            assert T.scalar_source_info() == tinfo, name
        # the source is as it was: the next event (after iteration 6) still matches the twin
        assert np.array_equal(A.scalar_source(), src.source)
        assert_source_equal(A, g, src, walls, "after the refused calls")
        A.step(2)
        g = host_run(B, g, [(2, {"scalar": True})], 3, src, walls)
        assert A.scalar_info()["updates"] == 2
        assert_source_equal(A, g, src, walls, "the next event")
    finally:
        for lat in (A, B, T):
            lat.close()


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
            src = L.ScalarSource(None, 0.1, (C.c_void_p * 2)(None, None), (C.c_void_p * 2)(None, None))
            assert s._lib.iblb_set_scalar_source(s.handle, C.byref(src)) == L.IBLB_ERR_STATE
            msg = s._lib.iblb_last_error(s.handle)
            assert msg and "group" in msg.decode()
            assert s.scalar_source_info() == {"decay": 0.0, "present": 0}
        group.step(2)
    finally:
        for s in slabs:
            s.close()
