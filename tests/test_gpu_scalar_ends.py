"""The scalar's open ends of iblb_set_scalar_ends on the GPU against tests/scalar_ends_ref.py (checked on the CPU by
tests/test_scalar_ends_ref.py) applied to what Lattice.fields returns for a twin lattice stepped in the pieces iblb_step
cuts its calls into.

The lattices, precisions, state and helpers are those of tests/test_gpu_scalar.py: 20 x 18, 37 x 23 (odd, fewer rows
than a wave) and 16 x 300 (the end lanes span two workgroups in y), f64 and f32 storage, tau 0.8.  Every comparison of
populations, totals and last is `==` (np.array_equal): the device does every operation of the rule once, rounded once,
and skips no term, which is what the numpy twin does; every accumulator entry has one writer per substep and the
substeps are ordered, so the sums carry no order of their own.  Lattices narrower than 16 columns (1 x 2, 2 x 3,
5 x 257) run in tests/test_gpu_scalar_matrix.py, with all nine pairs of end kinds under every pair of wall kinds.
"""
import ctypes as C

import numpy as np
import pytest

import scalar_ref as S
import scalar_source_ref as Q
import scalar_uptake_ref as U
import scalar_ends_ref as E
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_fields import BODY_FORCE
from test_gpu_scalar import LATTICES, PRECISIONS, TAU, WALLS, seeded_c0, velocity
from test_gpu_scalar import assert_scalar_equal
from test_gpu_tracers import moving_points, new_lattice

pytestmark = pytest.mark.gpu

VALUE_BELOW = WALLS["value below"]
NONE_SET = {"kind": None, "value": None, "present": 0, "substeps": 0}
NAMES = ["profile in, outflow", "outflow, value", "no flux both", "value both, a source, rates at both walls",
         "outflow both, value wall below"]
_CASES = {}


def cases(nx, ny):
    """{name: (Ends, Uptake or None, Source or None, walls)} for one size, computed once."""
    if (nx, ny) not in _CASES:
        rng = np.random.default_rng(nx * 977 + ny)
        prof0 = 0.5 + 0.4 * np.sin(2.0 * np.pi * (np.arange(ny) + 0.5) / ny)
        prof1 = rng.uniform(0.0, 1.0, ny)
        r0, r1 = rng.uniform(0.0, 2.0, (2, nx))
        field = rng.uniform(-2e-3, 4e-3, (ny, nx))
        f0, f1 = rng.uniform(-3e-3, 3e-3, (2, nx))
        for a in (prof0, prof1, r0, r1, field, f0, f1):
            a.setflags(write=False)
        _CASES[(nx, ny)] = {
            NAMES[0]: (E.Ends(("value", "outflow"), (0.0, 0.0), (prof0, None)), None, None, S.NO_FLUX_WALLS),
            NAMES[1]: (E.Ends(("outflow", "value"), (0.0, 0.6)), None, None, S.NO_FLUX_WALLS),
            NAMES[2]: (E.Ends(("noflux", "noflux")), None, None, S.NO_FLUX_WALLS),
            NAMES[3]: (E.Ends(("value", "value"), (0.8, 0.1), (None, prof1)), U.Uptake((r0, r1)),
                       Q.Source(field, 0.02, (f0, f1)), S.NO_FLUX_WALLS),
            NAMES[4]: (E.Ends(("outflow", "outflow")), None, None, VALUE_BELOW),
            "profile in, outflow, rates at both walls": (E.Ends(("value", "outflow"), (0.0, 0.0), (prof0, None)),
                                                         U.Uptake((r0, r1)), None, S.NO_FLUX_WALLS),
        }
    return _CASES[(nx, ny)]


def info_of(ends, substeps):
    return {"kind": ends.kind, "value": ends.value, "present": ends.present(), "substeps": substeps}


def host_run(B, g, sums, us, plan, stride, ends, up, src, walls):
    """Step the twin B in the pieces of `plan` and run the scalar's events with the ends on the host."""
    for n, due in plan:
        B.step(n)
        if due["scalar"]:
            g, sums, us = E.event(g, *velocity(B), TAU, stride, ends, sums, up, us, src, walls)
    return g, sums, us


def assert_sums_equal(got, sums, what):
    for k in range(2):
        assert np.array_equal(got["total"][k], sums.total[k]), (what, "total", k,
                                                                np.max(np.abs(got["total"][k] - sums.total[k])))
        assert np.array_equal(got["last"][k], sums.last[k]), (what, "last", k)
    assert got["substeps"] == sums.substeps, what


def assert_ends_equal(A, g, sums, us, src, walls, what):
    """Populations, the ends' sums, the uptake's sums where one is set (us not None), and the wall flux reader."""
    assert_scalar_equal(A, g, what)
    assert_sums_equal(A.scalar_ends(), sums, (what, "ends"))
    assert A.scalar_ends_info()["substeps"] == sums.substeps, what
    if us is not None:
        assert_sums_equal(A.scalar_uptake(), us, (what, "uptake"))
    # iblb_get_scalar_wall_flux keeps its expressions
    for got, want in zip(A.scalar_wall_flux(), Q.wall_flux(g, src if src is not None else Q.Source(), walls)):
        assert np.array_equal(got, want), (what, "wall flux")


def code_of(gpu, call):
    with pytest.raises(gpu.IblbError) as e:
        call()
    return e.value.code


def set_all(A, c0, stride, ends, up, src, walls):
    A.set_scalar(c0, tau=TAU, stride=stride, walls=walls)
    if src is not None:
        A.set_scalar_source(**src.kwargs())
    if up is not None:
        A.set_scalar_uptake(**up.kwargs())
    if ends is not None:
        A.set_scalar_ends(**ends.kwargs())


# ---- 1. the scalar with ends equals the twin -----------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("stride", [1, 5, 7])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_equals_the_twin(gpu, nx, ny, precision, stride, name):
    """step(2), the set, step(9); step(11): the events fall inside the calls and count on across them.  Twenty
    iterations: 20 substeps at the strides 1 and 5, two events of 7 at stride 7."""
    ends, up, src, walls = cases(nx, ny)[name]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    plain = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        B.step(2)
        plain.step(2)
        c0 = seeded_c0(nx, ny)
        set_all(A, c0, stride, ends, up, src, walls)
        set_all(plain, c0, stride, None, up, src, walls)
        assert A.scalar_ends_info() == info_of(ends, 0)
        assert plain.scalar_ends_info() == NONE_SET
        assert A.scalar_info()["updates"] == 0
        g, sums, us = S.equilibrium(c0, *velocity(B)), E.Sums(ny), None if up is None else U.Sums(nx)
        assert_ends_equal(A, g, sums, us, src, walls, "at the set")
        ta, tp = A.timing()["deep_launches"], plain.timing()["deep_launches"]
        t = 2
        for n in (9, 11):
            plan = S.pieces([n], t, scalar=(2, stride))
            assert any(d["scalar"] for _, d in plan)
            A.step(n)
            plain.step(n)
            g, sums, us = host_run(B, g, sums, us, plan, stride, ends, up, src, walls)
            t += n
            assert_ends_equal(A, g, sums, us, src, walls, f"after iteration {t}")
        assert A.scalar_info()["updates"] == 20 // stride
        assert A.scalar_ends()["substeps"] == sums.substeps == {1: 20, 5: 20, 7: 14}[stride]
        assert A.steps == B.steps == 22
        assert np.array_equal(A.populations(), B.populations())
        # the case is not empty: the run differs from the periodic one, and something crossed an end unless both
        # are closed
        assert not np.array_equal(plain.scalar_populations(), A.scalar_populations())
        assert np.any(sums.total != 0.0) == (name != "no flux both")
        if stride == 7:  # the ends keep the deep sweep between the events
            assert A.timing()["deep_launches"] - ta == plain.timing()["deep_launches"] - tp
    finally:
        for lat in (A, B, plain):
            lat.close()


# ---- 2. set, reset, replaced and removed in mid-run ----------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_changes_between_events(gpu, precision):
    """Stride 7, every call one event.  Periodic; ends set; source set, uptake set (the ends' totals carry on); reset;
    source removed; ends replaced with other kinds (their totals zeroed, the uptake's carry on); ends removed: the
    existing restatements again.  The twin is stepped in the same pieces: the deep launches are as many."""
    nx, ny = LATTICES[1]
    ends, up, src, walls = cases(nx, ny)[NAMES[3]]
    ends2 = cases(nx, ny)[NAMES[1]][0]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=7, walls=walls)
        g, sums, us = S.equilibrium(c0, *velocity(B)), E.Sums(ny), None
        ta, tb = A.timing(), B.timing()
        cur_ends = cur_up = cur_src = None

        def event(what):
            nonlocal g, sums, us
            A.step(7)
            B.step(7)
            g, sums, us = E.event(g, *velocity(B), TAU, 7, cur_ends, sums, cur_up, us, cur_src, walls)
            assert_scalar_equal(A, g, what)
            if cur_ends is not None:
                assert_ends_equal(A, g, sums, us, cur_src, walls, what)
            elif cur_up is not None:
                assert_sums_equal(A.scalar_uptake(), us, what)

        event("periodic")
        assert A.scalar_ends_info() == NONE_SET
        A.set_scalar_ends(**ends.kwargs())
        cur_ends = ends
        assert A.scalar_info()["updates"] == 1  # the set moves neither t0 nor the count
        assert_ends_equal(A, g, sums, us, None, walls, "at the set of the ends")
        event("the first event with the ends")
        assert sums.substeps == 7 and np.all(sums.total != 0.0)
        A.set_scalar_source(**src.kwargs())
        cur_src = src
        assert_sums_equal(A.scalar_ends(), sums, "at the set of the source")
        event("with the source")
        A.set_scalar_uptake(**up.kwargs())
        cur_up, us = up, U.Sums(nx)
        assert_sums_equal(A.scalar_ends(), sums, "at the set of the uptake")
        event("with the source and the uptake")
        assert sums.substeps == 21 and us.substeps == 7
        A.reset_scalar_ends()
        sums = E.Sums(ny)
        assert_sums_equal(A.scalar_ends(), sums, "at the reset")
        assert A.scalar_ends_info() == info_of(ends, 0)
        assert_sums_equal(A.scalar_uptake(), us, "the uptake at the ends' reset")
        event("after the reset")
        A.remove_scalar_source()
        cur_src = None
        assert_sums_equal(A.scalar_ends(), sums, "at the removal of the source")
        event("without the source")
        assert sums.substeps == 14 and us.substeps == 21
        A.set_scalar_ends(**ends2.kwargs())
        cur_ends, sums = ends2, E.Sums(ny)
        assert A.scalar_ends_info() == info_of(ends2, 0)
        assert_sums_equal(A.scalar_ends(), sums, "at the replacement")
        assert_sums_equal(A.scalar_uptake(), us, "the uptake at the replacement")
        event("with the second ends")
        assert np.all(sums.total != 0.0) and us.substeps == 28
        A.remove_scalar_uptake()
        cur_up, us = None, None
        assert_sums_equal(A.scalar_ends(), sums, "at the removal of the uptake")
        event("without the uptake")
        assert sums.substeps == 14
        A.remove_scalar_ends()
        cur_ends = None
        assert A.scalar_ends_info() == NONE_SET
        assert code_of(gpu, A.scalar_ends) == L.IBLB_ERR_STATE
        before = g
        event("periodic again")
        assert np.array_equal(g, S.event(before, *velocity(B), TAU, 7, walls))  # the existing restatement
        assert A.scalar_info()["updates"] == 9
        ta1, tb1 = A.timing(), B.timing()
        assert ta1["deep_launches"] - ta["deep_launches"] == tb1["deep_launches"] - tb["deep_launches"] > 0
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 3. with moving IB points --------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_with_moving_ib_points(gpu, precision):
    """Every call ends on an event, and the reference takes the lattice's own velocity read after the call: the owed
    IB force is in it."""
    nx, ny = LATTICES[1]
    stride = 3
    ends, up, src, walls = cases(nx, ny)[NAMES[3]]
    A = new_lattice(gpu, nx, ny, precision, with_points=True)
    try:
        A.set_lagrangian_steps(*moving_points(nx, ny, 12))
        c0 = seeded_c0(nx, ny)
        g, sums, us = S.equilibrium(c0, *velocity(A)), E.Sums(ny), U.Sums(nx)
        set_all(A, c0, stride, ends, up, src, walls)
        for _ in range(12 // stride):
            A.step(stride)
            g, sums, us = E.event(g, *velocity(A), TAU, stride, ends, sums, up, us, src, walls)
            assert_ends_equal(A, g, sums, us, src, walls, f"after iteration {A.steps}")
        assert A.scalar_info()["updates"] == 12 // stride and sums.substeps == 12
    finally:
        A.close()


# ---- 4. the budget on the device -----------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", LATTICES)
def test_budget_on_the_device(gpu, nx, ny):
    """Stride 7, three events, reactive no-flux walls and no bulk source: sum(C) of reduce(["c"]) changes by the sum
    of the ends' and the walls' totals, within scalar_ends_ref.budget_bound (the restatement alone stays within it at
    these sizes, kinds and magnitudes: tests/test_scalar_ends_ref.py)."""
    ends, up, src, walls = cases(nx, ny)["profile in, outflow, rates at both walls"]
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        set_all(A, seeded_c0(nx, ny), 7, ends, up, src, walls)
        s0, a0 = A.reduce(["c"])["c"].sum, np.sum(np.abs(A.scalar()))
        A.step(21)
        s1, a1 = A.reduce(["c"])["c"].sum, np.sum(np.abs(A.scalar()))
        got_e, got_u = A.scalar_ends(), A.scalar_uptake()
        assert got_e["substeps"] == got_u["substeps"] == 21
        at_ends = np.sum(got_e["total"][0] + got_e["total"][1])
        at_walls = np.sum(got_u["total"][0] + got_u["total"][1])
        bound = E.budget_bound(nx * ny, 21, nx, ny, max(a0, a1))
        print(f"{nx} x {ny}: d sum(C) {s1 - s0:.6e}, ends {at_ends:.6e}, walls {at_walls:.6e}, "
              f"|diff| {abs(s1 - s0 - at_ends - at_walls):.3e}, bound {bound:.3e}")
        assert abs((s1 - s0) - (at_ends + at_walls)) <= bound
        # either family left out misses
        assert abs((s1 - s0) - at_walls) > 1e6 * bound and abs((s1 - s0) - at_ends) > 1e6 * bound
    finally:
        A.close()


# ---- 5. lifecycle --------------------------------------------------------------------------------------------

def test_set_state_keeps_and_a_new_scalar_or_a_checkpoint_drops_the_ends(gpu, tmp_path):
    nx, ny = LATTICES[0]
    ends, up, src, walls = cases(nx, ny)[NAMES[0]]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        c0 = seeded_c0(nx, ny)
        set_all(A, c0, 3, ends, up, src, walls)
        g, sums = S.equilibrium(c0, *velocity(B)), E.Sums(ny)
        A.step(4)
        g, sums, _ = host_run(B, g, sums, None, S.pieces([4], 0, scalar=(0, 3)), 3, ends, up, src, walls)
        assert_ends_equal(A, g, sums, None, src, walls, "before the new state")
        rho, u = W.perturbed_state(nx, ny, 8)
        A.set_state(rho, u)
        B.set_state(rho, u)
        assert A.scalar_ends_info() == info_of(ends, 3)
        assert_sums_equal(A.scalar_ends(), sums, "at the new state")
        A.step(3)
        g, sums, _ = host_run(B, g, sums, None, S.pieces([3], 0, scalar=(0, 3)), 3, ends, up, src, walls)
        assert_ends_equal(A, g, sums, None, src, walls, "the first event of the new state")
        assert sums.substeps == 6
        # a replacement of the scalar drops the ends, and so does its removal
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        assert A.scalar_ends_info() == NONE_SET
        assert code_of(gpu, A.scalar_ends) == L.IBLB_ERR_STATE
        g = S.equilibrium(c0, *velocity(B))
        A.step(3)
        B.step(3)
        assert_scalar_equal(A, S.event(g, *velocity(B), TAU, 3, walls), "the periodic rule after the replacement")
        A.set_scalar_ends(**ends.kwargs())
        assert A.scalar_ends_info() == info_of(ends, 0)
        A.remove_scalar()
        assert A.scalar_ends_info() == NONE_SET
        assert code_of(gpu, lambda: A.set_scalar_ends()) == L.IBLB_ERR_STATE
        # a checkpoint holds neither
        set_all(A, c0, 3, ends, up, src, walls)
        ck = str(tmp_path / "ck")
        A.save_checkpoint(ck)
        A.load_checkpoint(ck)
        assert A.scalar_ends_info() == NONE_SET and A.scalar_info()["stride"] == 0
        A.step(5)
        B.step(5)
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 6. refusals leave everything as it was ------------------------------------------------------------------

def test_errors_leave_the_ends_as_they_were(gpu):
    nx, ny = LATTICES[0]
    ends, up, src, walls = cases(nx, ny)[NAMES[0]]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        # no scalar
        assert code_of(gpu, lambda: A.set_scalar_ends()) == L.IBLB_ERR_STATE
        assert A._lib.iblb_last_error(A.handle)
        assert code_of(gpu, A.remove_scalar_ends) == L.IBLB_ERR_STATE
        assert A.scalar_ends_info() == NONE_SET
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        # a scalar, no ends
        assert code_of(gpu, A.scalar_ends) == L.IBLB_ERR_STATE
        assert code_of(gpu, A.reset_scalar_ends) == L.IBLB_ERR_STATE
        A.remove_scalar_ends()  # nothing to remove: accepted, as iblb_set_scalar_uptake(NULL) is
        kind, value = (C.c_int * 2)(-3, -4), (C.c_double * 2)(-7.0, -8.0)
        assert A._lib.iblb_scalar_ends_info(A.handle, kind, value, None, None) == L.IBLB_OK
        assert list(kind) == [-3, -4] and list(value) == [-7.0, -8.0]  # none set: untouched
        A.set_scalar_ends(**ends.kwargs())
        g, sums = S.equilibrium(c0, *velocity(B)), E.Sums(ny)
        A.step(4)
        g, sums, _ = host_run(B, g, sums, None, S.pieces([4], 0, scalar=(0, 3)), 3, ends, up, src, walls)
        info = A.scalar_ends_info()
        assert info == info_of(ends, 3) and info["present"] == 1 | 2
        ok = np.full(ny, 0.1)
        at = lambda j, v: np.where(np.arange(ny) == j, v, 0.1)
        bad = {
            "a kind above the three": dict(kind=(3, "outflow")),
            "a negative kind": dict(kind=("value", -1)),
            "a NaN value at a value end": dict(kind=("value", "outflow"), value=(np.nan, 0.0)),
            "an infinite value at a value end": dict(kind=("noflux", "value"), value=(0.0, np.inf)),
            "a profile at an outflow end": dict(kind=("value", "outflow"), profile=(None, ok)),
            "a profile at a no-flux end beside a good one": dict(kind=("noflux", "value"), profile=(ok, ok)),
            "a NaN profile entry": dict(kind=("value", "outflow"), profile=(at(ny // 2, np.nan), None)),
            "an infinite last profile entry": dict(kind=("value", "value"), profile=(ok, at(ny - 1, -np.inf))),
        }
        for name, kw in bad.items():
            assert code_of(gpu, lambda: A.set_scalar_ends(**kw)) == L.IBLB_ERR_ARG, name
            assert A._lib.iblb_last_error(A.handle), name
            assert A.scalar_ends_info() == info, name
            assert_sums_equal(A.scalar_ends(), sums, name)
        assert A._lib.iblb_get_scalar_ends(A.handle, None, None, None, None, None) == L.IBLB_ERR_ARG
        # shape errors are raised before the call
        with pytest.raises(ValueError):
            A.set_scalar_ends(profile=(np.zeros(ny + 1), None))
        with pytest.raises(KeyError):
            A.set_scalar_ends(kind=("value", "sink"))
        assert A.scalar_ends_info() == info
        # single outputs
        n = C.c_longlong(-1)
        assert A._lib.iblb_get_scalar_ends(A.handle, None, None, None, None, C.byref(n)) == L.IBLB_OK and n.value == 3
        right = np.full(ny, -7.0)
        assert A._lib.iblb_get_scalar_ends(A.handle, None, right.ctypes.data_as(C.c_void_p), None, None, None) == L.IBLB_OK
        assert np.array_equal(right, sums.total[1])
        # the ends are as they were, profile included: the next event (after iteration 6) still matches the twin
        assert_ends_equal(A, g, sums, None, src, walls, "after the refused calls")
        A.step(2)
        g, sums, _ = host_run(B, g, sums, None, [(2, {"scalar": True})], 3, ends, up, src, walls)
        assert A.scalar_info()["updates"] == 2
        assert_ends_equal(A, g, sums, None, src, walls, "the next event")
    finally:
        A.close()
        B.close()


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
            ends = L.ScalarEnds((C.c_int * 2)(1, 2), (C.c_double * 2)(0.5, 0.0), (C.c_void_p * 2)(None, None))
            assert s._lib.iblb_set_scalar_ends(s.handle, C.byref(ends)) == L.IBLB_ERR_STATE
            msg = s._lib.iblb_last_error(s.handle)
            assert msg and "group" in msg.decode()
            assert s._lib.iblb_reset_scalar_ends(s.handle) == L.IBLB_ERR_STATE
            assert s.scalar_ends_info() == NONE_SET
        assert all(np.array_equal(s.populations(), b) for s, b in zip(slabs, before))
        group.step(2)
        twin.step(2)
        for s, t in zip(slabs, twins):
            assert s.steps == t.steps == 4 and np.array_equal(s.populations(), t.populations())
            assert not np.array_equal(s.populations(), before[slabs.index(s)])
    finally:
        for s in slabs + twins:
            s.close()
