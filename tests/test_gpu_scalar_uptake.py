"""The scalar's uptake of iblb_set_scalar_uptake on the GPU against tests/scalar_uptake_ref.py (checked on the CPU by
tests/test_scalar_uptake_ref.py) applied to what Lattice.fields returns for a twin lattice stepped in the pieces
iblb_step cuts its calls into.

The lattices, precisions, state and helpers are those of tests/test_gpu_scalar.py: 20 x 18, 37 x 23 (odd, fewer rows
than a wave) and 16 x 300 (the top-wall lanes sit in the second workgroup), f64 and f32 storage, tau 0.8.  Every
comparison of populations, totals and last is `==` (np.array_equal): the device does every operation of the rule once,
rounded once, and skips no term, which is what the numpy twin does; every accumulator entry has one writer per substep
and the substeps are ordered, so the sums carry no order of their own.
"""
import ctypes as C

import numpy as np
import pytest

import scalar_ref as S
import scalar_source_ref as Q
import scalar_uptake_ref as U
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_fields import BODY_FORCE
from test_gpu_scalar import LATTICES, PRECISIONS, TAU, WALLS, seeded_c0, velocity
from test_gpu_scalar import assert_scalar_equal
from test_gpu_tracers import moving_points, new_lattice

pytestmark = pytest.mark.gpu

VALUE_BELOW = WALLS["value below"]
VALUE_ABOVE = ((S.NOFLUX, 0.0), (S.VALUE, 0.25))
VALUE_BOTH = ((S.VALUE, 0.25), (S.VALUE, 0.1))
NONE_SET = {"present": 0, "substeps": 0}
_CASES = {}


def cases(nx, ny):
    """{name: (Uptake, Source or None, walls)} for one size, computed once."""
    if (nx, ny) not in _CASES:
        rng = np.random.default_rng(nx * 991 + ny)
        r0, r1 = rng.uniform(0.0, 2.0, (2, nx))
        r0[[0, nx // 2, nx - 1]] = (0.0, 1.0 / 3.0, 50.0)
        r1[[1, nx // 3, nx - 2]] = (50.0, 0.0, 1.0 / 3.0)
        field = rng.uniform(-2e-3, 4e-3, (ny, nx))
        f0, f1 = rng.uniform(-3e-3, 3e-3, (2, nx))
        v1 = 0.25 + 0.2 * np.sin(2.0 * np.pi * np.arange(nx) / nx)
        for a in (r0, r1, field, f0, f1, v1):
            a.setflags(write=False)
        _CASES[(nx, ny)] = {
            "rates below": (U.Uptake((r0, None)), None, S.NO_FLUX_WALLS),
            "rates at both walls, a source": (U.Uptake((r0, r1)), Q.Source(field, 0.02, (f0, f1)), S.NO_FLUX_WALLS),
            "value profile above, rate below": (U.Uptake((r0, None)), Q.Source(wall_value=(None, v1)), VALUE_ABOVE),
            "accumulate only": (U.Uptake(), None, VALUE_BOTH),
            "rates at both walls": (U.Uptake((r0, r1)), None, S.NO_FLUX_WALLS),
        }
    return _CASES[(nx, ny)]


def host_run(B, g, sums, plan, stride, up, src, walls):
    """Step the twin B in the pieces of `plan` and run the scalar's events with the uptake on the host."""
    for n, due in plan:
        B.step(n)
        if due["scalar"]:
            g, sums = U.event(g, *velocity(B), TAU, stride, up, sums, src, walls)
    return g, sums


def assert_sums_equal(A, sums, what):
    got = A.scalar_uptake()
    for k in range(2):
        assert np.array_equal(got["total"][k], sums.total[k]), (what, "total", k,
                                                                np.max(np.abs(got["total"][k] - sums.total[k])))
        assert np.array_equal(got["last"][k], sums.last[k]), (what, "last", k)
    assert got["substeps"] == sums.substeps, what
    assert A.scalar_uptake_info()["substeps"] == sums.substeps, what


def assert_uptake_equal(A, g, sums, src, walls, what):
    assert_scalar_equal(A, g, what)
    assert_sums_equal(A, sums, what)
    # iblb_get_scalar_wall_flux keeps its expressions: the uptake's loss is not in it
    for got, want in zip(A.scalar_wall_flux(), Q.wall_flux(g, src if src is not None else Q.Source(), walls)):
        assert np.array_equal(got, want), (what, "wall flux")


def code_of(gpu, call):
    with pytest.raises(gpu.IblbError) as e:
        call()
    return e.value.code


def set_all(A, c0, stride, up, src, walls):
    A.set_scalar(c0, tau=TAU, stride=stride, walls=walls)
    if src is not None:
        A.set_scalar_source(**src.kwargs())
    if up is not None:
        A.set_scalar_uptake(**up.kwargs())


# ---- 1. the scalar with an uptake equals the twin ------------------------------------------------------------

@pytest.mark.parametrize("name", ["rates below", "rates at both walls, a source", "value profile above, rate below",
                                  "accumulate only"])
@pytest.mark.parametrize("stride", [1, 5, 7])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_equals_the_twin(gpu, nx, ny, precision, stride, name):
    """step(9); step(11) with the scalar, its source and its uptake set at t0 = 2: the events fall inside the calls
    and count on across them.  Twenty iterations: 20 substeps at the strides 1 and 5, two events of 7 at stride 7."""
    up, src, walls = cases(nx, ny)[name]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    plain = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        B.step(2)
        plain.step(2)
        c0 = seeded_c0(nx, ny)
        set_all(A, c0, stride, up, src, walls)
        set_all(plain, c0, stride, None, src, walls)
        assert A.scalar_uptake_info() == {"present": up.present(), "substeps": 0}
        assert A.scalar_info()["updates"] == 0
        g, sums = S.equilibrium(c0, *velocity(B)), U.Sums(nx)
        assert_uptake_equal(A, g, sums, src, walls, "at the set")
        t = 2
        for n in (9, 11):
            plan = S.pieces([n], t, scalar=(2, stride))
            assert any(d["scalar"] for _, d in plan)
            A.step(n)
            plain.step(n)
            g, sums = host_run(B, g, sums, plan, stride, up, src, walls)
            t += n
            assert_uptake_equal(A, g, sums, src, walls, f"after iteration {t}")
        assert A.scalar_info()["updates"] == 20 // stride
        assert A.scalar_uptake()["substeps"] == {1: 20, 5: 20, 7: 14}[stride]
        assert A.steps == B.steps == 22
        assert np.array_equal(A.populations(), B.populations())
        # the case is not empty: the uptake changed C and something crossed a wall, unless it only accumulates,
        # and then the run is the one without an uptake
        same = np.array_equal(plain.scalar_populations(), A.scalar_populations())
        assert same == (name == "accumulate only")
        assert np.any(sums.total != 0.0)
    finally:
        for lat in (A, B, plain):
            lat.close()


# ---- 2. set, reset, replaced and removed in mid-run ----------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_changes_between_events(gpu, precision):
    """Stride 7, every call one event.  Without an uptake; uptake set; source set (totals carry on); reset; source
    removed (totals carry on); uptake replaced (totals zeroed); uptake removed.  The twin is stepped in the same
    pieces: the deep launches are as many."""
    nx, ny = LATTICES[1]
    up, src, walls = cases(nx, ny)["rates at both walls, a source"]
    up2 = U.Uptake((None, up.rate[0]))
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=7, walls=walls)
        g, sums = S.equilibrium(c0, *velocity(B)), U.Sums(nx)
        ta, tb = A.timing(), B.timing()
        cur_up = cur_src = None

        def event(what):
            nonlocal g, sums
            A.step(7)
            B.step(7)
            g, sums = U.event(g, *velocity(B), TAU, 7, cur_up, sums, cur_src, walls)
            assert_scalar_equal(A, g, what)
            if cur_up is not None:
                assert_uptake_equal(A, g, sums, cur_src, walls, what)

        event("without an uptake")
        assert A.scalar_uptake_info() == NONE_SET
        A.set_scalar_uptake(**up.kwargs())
        cur_up = up
        assert A.scalar_info()["updates"] == 1  # the set moves neither t0 nor the count
        assert_uptake_equal(A, g, sums, None, walls, "at the set of the uptake")
        event("the first event with the uptake")
        assert sums.substeps == 7
        A.set_scalar_source(**src.kwargs())
        cur_src = src
        assert_sums_equal(A, sums, "at the set of the source")
        event("with the source")
        assert sums.substeps == 14
        A.reset_scalar_uptake()
        sums = U.Sums(nx)
        assert_sums_equal(A, sums, "at the reset")
        assert A.scalar_uptake_info() == {"present": up.present(), "substeps": 0}
        event("after the reset")
        A.remove_scalar_source()
        cur_src = None
        assert_sums_equal(A, sums, "at the removal of the source")
        event("without the source")
        assert sums.substeps == 14 and np.all(sums.total[0, 1:] != 0.0)
        A.set_scalar_uptake(**up2.kwargs())
        cur_up, sums = up2, U.Sums(nx)
        assert A.scalar_uptake_info() == {"present": 1 | 4, "substeps": 0}
        assert_sums_equal(A, sums, "at the replacement")
        event("with the second uptake")
        assert np.array_equal(sums.total[0], np.zeros(nx)) and np.any(sums.total[1] != 0.0)
        A.remove_scalar_uptake()
        cur_up = None
        assert A.scalar_uptake_info() == NONE_SET
        assert code_of(gpu, A.scalar_uptake) == L.IBLB_ERR_STATE
        event("without an uptake again")
        assert A.scalar_info()["updates"] == 7
        ta1, tb1 = A.timing(), B.timing()
        assert ta1["deep_launches"] - ta["deep_launches"] == tb1["deep_launches"] - tb["deep_launches"] > 0
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 3. with moving IB points --------------------------------------------------------------------------------

def test_with_moving_ib_points(gpu):
    """Every call ends on an event, and the reference takes the lattice's own velocity read after the call: the owed
    IB force is in it."""
    nx, ny = LATTICES[1]
    stride = 3
    up, src, walls = cases(nx, ny)["rates at both walls, a source"]
    A = new_lattice(gpu, nx, ny, "f64", with_points=True)
    try:
        A.set_lagrangian_steps(*moving_points(nx, ny, 12))
        c0 = seeded_c0(nx, ny)
        g, sums = S.equilibrium(c0, *velocity(A)), U.Sums(nx)
        set_all(A, c0, stride, up, src, walls)
        for _ in range(12 // stride):
            A.step(stride)
            g, sums = U.event(g, *velocity(A), TAU, stride, up, sums, src, walls)
            assert_uptake_equal(A, g, sums, src, walls, f"after iteration {A.steps}")
        assert A.scalar_info()["updates"] == 12 // stride and sums.substeps == 12
    finally:
        A.close()


# ---- 4. the budget on the device -----------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", LATTICES)
def test_budget_on_the_device(gpu, nx, ny):
    """Stride 7, three events, no bulk source: sum(C) of reduce(["c"]) changes by the sum of the totals, within the
    bound of the CPU check (scalar_uptake_ref.budget_bound)."""
    up, src, walls = cases(nx, ny)["rates at both walls"]
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        set_all(A, seeded_c0(nx, ny), 7, up, src, walls)
        s0, a0 = A.reduce(["c"])["c"].sum, np.sum(np.abs(A.scalar()))
        A.step(21)
        s1, a1 = A.reduce(["c"])["c"].sum, np.sum(np.abs(A.scalar()))
        got = A.scalar_uptake()
        assert got["substeps"] == 21
        want = np.sum(got["total"][0] + got["total"][1])
        bound = U.budget_bound(nx * ny, 21, nx, max(a0, a1))
        print(f"{nx} x {ny}: d sum(C) {s1 - s0:.6e}, totals {want:.6e}, |diff| {abs(s1 - s0 - want):.3e}, "
              f"bound {bound:.3e}")
        assert want < 0.0 and abs((s1 - s0) - want) <= bound
        assert abs((s1 - s0) - np.sum(got["total"][0])) > 1e6 * bound  # one wall left out misses
    finally:
        A.close()


# ---- 5. a huge rate is the value wall at zero ----------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_huge_rate_equals_the_value_wall_at_zero(gpu, precision):
    nx, ny = LATTICES[1]
    A = new_lattice(gpu, nx, ny, precision)
    V = new_lattice(gpu, nx, ny, precision)
    try:
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=5)
        A.set_scalar_uptake(rate=(np.full(nx, 1e300), None))
        V.set_scalar(c0, tau=TAU, stride=5, walls=((S.VALUE, 0.0), (S.NOFLUX, 0.0)))
        V.set_scalar_uptake()
        A.step(10)
        V.step(10)
        assert np.array_equal(A.scalar_populations(), V.scalar_populations())
        a, v = A.scalar_uptake(), V.scalar_uptake()
        assert a["substeps"] == v["substeps"] == 10
        # a = 2: l = 2 q, net = 0 - 2 q; the value wall: g3' = 0 - q, net = g3' - q: the same amounts
        assert np.array_equal(a["total"][0], v["total"][0]) and np.all(a["total"][0] < 0)
        assert np.array_equal(a["last"][0], v["last"][0])
        assert np.array_equal(v["last"][0], V.scalar_wall_flux()[0])
    finally:
        A.close()
        V.close()


# ---- 6. lifecycle --------------------------------------------------------------------------------------------

def test_set_state_keeps_and_a_new_scalar_or_a_checkpoint_drops_the_uptake(gpu, tmp_path):
    nx, ny = LATTICES[0]
    up, src, walls = cases(nx, ny)["value profile above, rate below"]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        c0 = seeded_c0(nx, ny)
        set_all(A, c0, 3, up, src, walls)
        g, sums = S.equilibrium(c0, *velocity(B)), U.Sums(nx)
        A.step(4)
        g, sums = host_run(B, g, sums, S.pieces([4], 0, scalar=(0, 3)), 3, up, src, walls)
        assert_uptake_equal(A, g, sums, src, walls, "before the new state")
        rho, u = W.perturbed_state(nx, ny, 8)
        A.set_state(rho, u)
        B.set_state(rho, u)
        assert A.scalar_uptake_info() == {"present": up.present(), "substeps": 3}
        assert_sums_equal(A, sums, "at the new state")
        A.step(3)
        g, sums = host_run(B, g, sums, S.pieces([3], 0, scalar=(0, 3)), 3, up, src, walls)  # the plan restarts from 0
        assert_uptake_equal(A, g, sums, src, walls, "the first event of the new state")
        assert sums.substeps == 6
        # a replacement of the scalar drops the uptake, and so does its removal
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        assert A.scalar_uptake_info() == NONE_SET
        assert code_of(gpu, A.scalar_uptake) == L.IBLB_ERR_STATE
        g = S.equilibrium(c0, *velocity(B))
        A.step(3)
        B.step(3)
        assert_scalar_equal(A, S.event(g, *velocity(B), TAU, 3, walls), "the old rule after the replacement")
        A.set_scalar_uptake(**up.kwargs())
        assert A.scalar_uptake_info() == {"present": up.present(), "substeps": 0}
        A.remove_scalar()
        assert A.scalar_uptake_info() == NONE_SET
        assert code_of(gpu, lambda: A.set_scalar_uptake()) == L.IBLB_ERR_STATE
        # a checkpoint holds neither
        set_all(A, c0, 3, up, src, walls)
        ck = str(tmp_path / "ck")
        A.save_checkpoint(ck)
        A.load_checkpoint(ck)
        assert A.scalar_uptake_info() == NONE_SET and A.scalar_info()["stride"] == 0
        A.step(5)
        B.step(5)
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 7. refusals leave everything as it was ------------------------------------------------------------------

def test_errors_leave_the_uptake_as_it_was(gpu):
    nx, ny = LATTICES[0]
    up, src, walls = cases(nx, ny)["value profile above, rate below"]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        # no scalar
        assert code_of(gpu, lambda: A.set_scalar_uptake()) == L.IBLB_ERR_STATE
        assert A._lib.iblb_last_error(A.handle)
        assert code_of(gpu, A.remove_scalar_uptake) == L.IBLB_ERR_STATE
        assert A.scalar_uptake_info() == NONE_SET
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        # a scalar, no uptake
        assert code_of(gpu, A.scalar_uptake) == L.IBLB_ERR_STATE
        assert code_of(gpu, A.reset_scalar_uptake) == L.IBLB_ERR_STATE
        A.remove_scalar_uptake()  # nothing to remove: accepted, as iblb_set_scalar_source(NULL) is
        A.set_scalar_source(**src.kwargs())
        A.set_scalar_uptake(**up.kwargs())
        g, sums = S.equilibrium(c0, *velocity(B)), U.Sums(nx)
        A.step(4)
        g, sums = host_run(B, g, sums, S.pieces([4], 0, scalar=(0, 3)), 3, up, src, walls)
        info = A.scalar_uptake_info()
        assert info == {"present": 1 | 2, "substeps": 3}
        ok = np.full(nx, 0.1)
        at = lambda v: np.where(np.arange(nx) == nx // 2, v, 0.1)
        bad = {
            "a NaN rate": (at(np.nan), None),
            "an infinite rate": (at(np.inf), None),
            "a negative rate": (at(-1e-300), None),
            "a negative rate in the last entry": (np.where(np.arange(nx) == nx - 1, -1.0, 0.1), None),
            "a rate on a _VALUE wall": (None, ok),
            "a rate on a _VALUE wall beside a good one": (ok, ok),
        }
        for name, rate in bad.items():
            assert code_of(gpu, lambda: A.set_scalar_uptake(rate=rate)) == L.IBLB_ERR_ARG, name
            assert A._lib.iblb_last_error(A.handle), name
            assert A.scalar_uptake_info() == info, name
            assert_sums_equal(A, sums, name)
        assert A._lib.iblb_get_scalar_uptake(A.handle, None, None, None, None, None) == L.IBLB_ERR_ARG
        # shape errors are raised before the call
        with pytest.raises(ValueError):
            A.set_scalar_uptake(rate=(np.zeros(nx + 1), None))
        with pytest.raises(ValueError):
            A.set_scalar_uptake(rate=(None, np.zeros(nx - 1)))
        assert A.scalar_uptake_info() == info
        # single outputs
        n = C.c_longlong(-1)
        assert A._lib.iblb_get_scalar_uptake(A.handle, None, None, None, None, C.byref(n)) == L.IBLB_OK and n.value == 3
        top = np.full(nx, -7.0)
        assert A._lib.iblb_get_scalar_uptake(A.handle, None, top.ctypes.data_as(C.c_void_p), None, None, None) == L.IBLB_OK
        assert np.array_equal(top, sums.total[1])
        # the uptake is as it was, rates included: the next event (after iteration 6) still matches the twin
        assert_uptake_equal(A, g, sums, src, walls, "after the refused calls")
        A.step(2)
        g, sums = host_run(B, g, sums, [(2, {"scalar": True})], 3, up, src, walls)
        assert A.scalar_info()["updates"] == 2
        assert_uptake_equal(A, g, sums, src, walls, "the next event")
    finally:
        A.close()
        B.close()


# ---- 8. the slabs of a group ---------------------------------------------------------------------------------

def test_a_slab_of_a_group_is_refused(gpu):
    """Both slabs refuse every call with IBLB_ERR_STATE, and the group then steps as a twin group that was never
    asked: no IB points, so the two runs are equal bit for bit."""
    nx, ny = LATTICES[0]
    rho, u = W.perturbed_state(nx, ny, 7)
    slabs, twins = [], []
    for made in (slabs, twins):
        for xb, xc in gpu.plan_slabs(nx, 2):
            s = gpu.Lattice(nx, ny, W.TAU, W.TAU2, body_force=BODY_FORCE, x_begin=xb, x_count=xc)
            made.append(s)
            s.set_state(gpu.split_state(rho, 1, nx, ny, xb, xc), gpu.split_state(u, 2, nx, ny, xb, xc))
    try:
        group, twin = gpu.LocalGroup(slabs), gpu.LocalGroup(twins)
        group.step(2)
        twin.step(2)
        before = [s.populations() for s in slabs]
        for s in slabs:
            up = L.ScalarUptake((C.c_void_p * 2)(None, None))
            assert s._lib.iblb_set_scalar_uptake(s.handle, C.byref(up)) == L.IBLB_ERR_STATE
            msg = s._lib.iblb_last_error(s.handle)
            assert msg and "group" in msg.decode()
            assert s._lib.iblb_reset_scalar_uptake(s.handle) == L.IBLB_ERR_STATE
            assert s.scalar_uptake_info() == NONE_SET
        assert all(np.array_equal(s.populations(), b) for s, b in zip(slabs, before))
        group.step(2)
        twin.step(2)
        for s, t in zip(slabs, twins):
            assert s.steps == t.steps == 4 and np.array_equal(s.populations(), t.populations())
            assert not np.array_equal(s.populations(), before[slabs.index(s)])
    finally:
        for s in slabs + twins:
            s.close()
