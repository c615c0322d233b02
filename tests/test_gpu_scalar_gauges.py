"""The scalar's transport gauges of iblb_set_scalar_gauges on the GPU against tests/scalar_gauges_ref.py (checked on the
CPU by tests/test_scalar_gauges_ref.py) applied to what Lattice.fields returns for a twin lattice stepped in the pieces
iblb_step cuts its calls into.

The lattices, precisions, state and helpers are those of tests/test_gpu_scalar.py: 20 x 18, 37 x 23 (odd, fewer rows
than a wave) and 16 x 300 (two workgroups in y), f64 and f32 storage, tau 0.8.  Every comparison with the twin is `==`
(np.array_equal): the device adds every p_i once, rounded once, from one writer per entry and substep.  The positions
reach the edges on every size: stations 0, two adjacent columns (a lane then writes `right` of its own station and
`left` of the previous one) and nx - 1 (the wrap: column 0 writes its `left`); levels 0, two adjacent rows and ny - 2,
and on 16 x 300 also 63 and 255, whose `up` and `down` writers sit in different waves and in different workgroups.
Lattices narrower than 16 columns (1 x 2, 2 x 3, 5 x 257) run in tests/test_gpu_scalar_matrix.py, with every combination
of a source, an uptake, open ends and gauges under every pair of wall kinds.
"""
import ctypes as C

import numpy as np
import pytest

import scalar_ref as S
import scalar_uptake_ref as U
import scalar_ends_ref as E
import scalar_gauges_ref as G
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_fields import BODY_FORCE
from test_gpu_scalar import LATTICES, PRECISIONS, TAU, seeded_c0, velocity
from test_gpu_scalar import assert_scalar_equal
from test_gpu_scalar_ends import cases as ends_cases, code_of, set_all
from test_gpu_tracers import moving_points, new_lattice

pytestmark = pytest.mark.gpu

NONE_SET = {"stations": (), "levels": (), "substeps": 0}
NAMES = ["periodic", "open ends", "a source, an uptake and open ends"]


def positions(nx, ny):
    levels = (0, ny // 2 - 1, ny // 2, ny - 2)
    if ny == 300:
        levels = (0, 63, 149, 150, 255, 298)
    return G.Gauges((0, nx // 2, nx // 2 + 1, nx - 1), levels)


def cases(nx, ny):
    """{name: (Ends or None, Uptake or None, Source or None, walls)}: those of tests/test_gpu_scalar_ends.py."""
    c = ends_cases(nx, ny)
    return {NAMES[0]: (None, None, None, S.NO_FLUX_WALLS), NAMES[1]: c["profile in, outflow"],
            NAMES[2]: c["value both, a source, rates at both walls"]}


class Twin:
    """The host's side of one run: the populations and every family of sums, advanced by scalar_gauges_ref.event."""

    def __init__(self, B, c0, nx, ny, stride, gauges, ends, up, src, walls):
        self.B, self.stride, self.gauges = B, stride, gauges
        self.ends, self.up, self.src, self.walls = ends, up, src, walls
        self.nx, self.ny = nx, ny
        self.g = S.equilibrium(c0, *velocity(B))
        self.sums = None if gauges is None else G.Sums(gauges, nx, ny)
        self.es = None if ends is None else E.Sums(ny)
        self.us = None if up is None else U.Sums(nx)

    def event(self):
        self.g, self.sums, self.es, self.us = G.event(self.g, *velocity(self.B), TAU, self.stride, self.gauges,
                                                      self.sums, self.ends, self.es, self.up, self.us, self.src,
                                                      self.walls)

    def run(self, plan):
        """Step the fluid twin in the pieces of `plan` and run the scalar's events on the host."""
        for n, due in plan:
            self.B.step(n)
            if due["scalar"]:
                self.event()


def assert_gauges_equal(A, gauges, sums, what):
    got = A.scalar_gauges()
    for name in ("right", "left", "up", "down"):
        want = getattr(sums, name)
        assert got[name].shape == want.shape, (what, name)
        assert np.array_equal(got[name], want), (what, name, np.max(np.abs(got[name] - want)))
    assert got["substeps"] == sums.substeps, what
    assert A.scalar_gauges_info() == gauges.info(sums.substeps), what


def assert_same_as_without(A, plain, what):
    """The gauges change nothing: populations, the uptake's and the ends' totals equal those of the lattice without."""
    assert np.array_equal(A.scalar_populations(), plain.scalar_populations()), what
    for info, get in (("scalar_uptake_info", "scalar_uptake"), ("scalar_ends_info", "scalar_ends")):
        assert getattr(A, info)() == getattr(plain, info)(), (what, info)
        if getattr(A, info)()["present"]:
            a, p = getattr(A, get)(), getattr(plain, get)()
            for k in range(2):
                assert np.array_equal(a["total"][k], p["total"][k]) and np.array_equal(a["last"][k], p["last"][k]), (what, get)
            assert a["substeps"] == p["substeps"], (what, get)


# ---- 1. the gauges equal the twin, and change nothing --------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("stride", [1, 5, 7])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_equals_the_twin(gpu, nx, ny, precision, stride, name):
    """step(2), the set, step(9); step(11): the events fall inside the calls and count on across them.  Twenty
    iterations: 20 substeps at the strides 1 and 5, two events of 7 at stride 7."""
    ends, up, src, walls = cases(nx, ny)[name]
    ga = positions(nx, ny)
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    plain = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        B.step(2)
        plain.step(2)
        c0 = seeded_c0(nx, ny)
        set_all(A, c0, stride, ends, up, src, walls)
        set_all(plain, c0, stride, ends, up, src, walls)
        assert A.scalar_gauges_info() == NONE_SET
        A.set_scalar_gauges(**ga.kwargs())
        assert plain.scalar_gauges_info() == NONE_SET and A.scalar_info()["updates"] == 0
        twin = Twin(B, c0, nx, ny, stride, ga, ends, up, src, walls)
        assert_gauges_equal(A, ga, twin.sums, "at the set")
        ta, tp = A.timing()["deep_launches"], plain.timing()["deep_launches"]
        t = 2
        for n in (9, 11):
            plan = S.pieces([n], t, scalar=(2, stride))
            assert any(d["scalar"] for _, d in plan)
            A.step(n)
            plain.step(n)
            twin.run(plan)
            t += n
            assert_gauges_equal(A, ga, twin.sums, f"after iteration {t}")
            assert_scalar_equal(A, twin.g, f"after iteration {t}")
            assert_same_as_without(A, plain, f"after iteration {t}")
        assert A.scalar_info()["updates"] == 20 // stride
        assert twin.sums.substeps == {1: 20, 5: 20, 7: 14}[stride]
        assert A.steps == B.steps == 22 and np.array_equal(A.populations(), B.populations())
        # the case is not empty: every link carried something, but for the last column's under open ends
        last = len(ga.stations) - 1
        for k in range(last + 1):
            closed = ends is not None and k == last
            assert np.all((twin.sums.right[k] == 0.0) == closed) and np.all((twin.sums.left[k] == 0.0) == closed), k
        assert np.all(twin.sums.up != 0.0) and np.all(twin.sums.down != 0.0)
        if stride == 7:  # the gauges keep the deep sweep between the events
            assert A.timing()["deep_launches"] - ta == plain.timing()["deep_launches"] - tp
    finally:
        for lat in (A, B, plain):
            lat.close()


# ---- 2. set, reset, replaced and removed in mid-run ----------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_changes_between_events(gpu, precision):
    """Stride 7, every call one event.  No gauges; set; reset; replaced with other positions (the totals zeroed); ends,
    a source and an uptake set (the gauges' totals carry on); removed: the rule in force alone again."""
    nx, ny = LATTICES[1]
    ends, up, src, walls = cases(nx, ny)[NAMES[2]]
    ga, ga2 = positions(nx, ny), G.Gauges((3,), ())
    ga3 = G.Gauges((), (1, 2, 3))
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=7, walls=walls)
        twin = Twin(B, c0, nx, ny, 7, None, None, None, None, walls)

        def event(what):
            A.step(7)
            B.step(7)
            twin.event()
            assert_scalar_equal(A, twin.g, what)
            if twin.gauges is not None:
                assert_gauges_equal(A, twin.gauges, twin.sums, what)

        def use(gauges):
            twin.gauges, twin.sums = gauges, None if gauges is None else G.Sums(gauges, nx, ny)

        event("no gauges")
        A.set_scalar_gauges(**ga.kwargs())
        use(ga)
        assert A.scalar_info()["updates"] == 1  # the set moves neither t0 nor the count
        assert_gauges_equal(A, ga, twin.sums, "at the set")
        event("the first event with the gauges")
        assert twin.sums.substeps == 7 and np.all(twin.sums.right != 0.0)
        A.reset_scalar_gauges()
        use(ga)
        assert_gauges_equal(A, ga, twin.sums, "at the reset")
        event("after the reset")
        A.set_scalar_gauges(**ga2.kwargs())
        use(ga2)
        assert_gauges_equal(A, ga2, twin.sums, "at the replacement")
        got = A.scalar_gauges()
        assert got["right"].shape == (1, ny) and got["up"].shape == (0, nx)
        event("one station, no level")
        A.set_scalar_gauges(**ga3.kwargs())
        use(ga3)
        event("three levels, no station")
        assert twin.sums.substeps == 7
        A.set_scalar_ends(**ends.kwargs())
        twin.ends, twin.es = ends, E.Sums(ny)
        assert_gauges_equal(A, ga3, twin.sums, "at the set of the ends")
        event("with the ends")
        A.set_scalar_source(**src.kwargs())
        A.set_scalar_uptake(**up.kwargs())
        twin.src, twin.up, twin.us = src, up, U.Sums(nx)
        assert_gauges_equal(A, ga3, twin.sums, "at the set of the source and the uptake")
        event("with the ends, the source and the uptake")
        assert twin.sums.substeps == 21 and twin.es.substeps == 14 and twin.us.substeps == 7
        A.set_scalar_gauges(**ga.kwargs())
        use(ga)
        for a, want in ((A.scalar_ends(), twin.es), (A.scalar_uptake(), twin.us)):  # the set keeps the other totals
            assert a["substeps"] == want.substeps
            assert np.array_equal(a["total"][0], want.total[0]) and np.array_equal(a["total"][1], want.total[1])
        event("the first positions again, everything set")
        A.remove_scalar_gauges()
        use(None)
        assert A.scalar_gauges_info() == NONE_SET
        assert code_of(gpu, A.scalar_gauges) == L.IBLB_ERR_STATE
        event("without gauges again")
        assert A.scalar_info()["updates"] == 9 and A.scalar_ends()["substeps"] == 28
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
    ends, up, src, walls = cases(nx, ny)[NAMES[2]]
    ga = positions(nx, ny)
    A = new_lattice(gpu, nx, ny, precision, with_points=True)
    try:
        A.set_lagrangian_steps(*moving_points(nx, ny, 12))
        c0 = seeded_c0(nx, ny)
        twin = Twin(A, c0, nx, ny, stride, ga, ends, up, src, walls)
        set_all(A, c0, stride, ends, up, src, walls)
        A.set_scalar_gauges(**ga.kwargs())
        for _ in range(12 // stride):
            A.step(stride)
            twin.event()
            assert_scalar_equal(A, twin.g, f"after iteration {A.steps}")
            assert_gauges_equal(A, ga, twin.sums, f"after iteration {A.steps}")
        assert A.scalar_info()["updates"] == 12 // stride and twin.sums.substeps == 12
    finally:
        A.close()


# ---- 4. the budget on the device -----------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", LATTICES)
def test_box_budget_on_the_device(gpu, nx, ny):
    """Stride 7, three events, open ends, reactive no-flux walls, no bulk source.  The box between the first two
    stations and the first two levels: d sum(C) is the four gauges' nets.  The strip of full height right of the third
    station: the station's net, the right end's total (the station at nx - 1 reads nothing there) and the walls' totals
    over its columns.  Both within scalar_gauges_ref.budget_bound (the restatement alone stays within it:
    tests/test_scalar_gauges_ref.py)."""
    ends, up, src, walls = ends_cases(nx, ny)["profile in, outflow, rates at both walls"]
    ga = positions(nx, ny)
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        set_all(A, seeded_c0(nx, ny), 7, ends, up, src, walls)
        A.set_scalar_gauges(**ga.kwargs())
        C0 = A.scalar()
        A.step(21)
        C1 = A.scalar()
        got, got_e, got_u = A.scalar_gauges(), A.scalar_ends(), A.scalar_uptake()
        assert got["substeps"] == got_e["substeps"] == got_u["substeps"] == 21
        sums = G.Sums(ga, nx, ny, got["right"], got["left"], got["up"], got["down"], 21)
        (X0, X1, X2, X3), (Y0, Y1) = ga.stations, ga.levels[:2]
        for what, cols, rows in (("box", (X0, X1), (Y0, Y1)), ("strip", (X2, None), (None, None))):
            xs = slice(cols[0] + 1, nx if cols[1] is None else cols[1] + 1)
            ys = slice(0 if rows[0] is None else rows[0] + 1, ny if rows[1] is None else rows[1] + 1)
            entered, n_st, n_lv = G.box_net(ga, sums, cols, rows, nx, ny)
            without = 0.0
            if what == "strip":
                without = np.sum(got_e["total"][1]) + np.sum(got_u["total"][0][xs]) + np.sum(got_u["total"][1][xs])
            d = np.sum(C1[ys, xs]) - np.sum(C0[ys, xs])
            scale = max(np.sum(np.abs(C0[ys, xs])), np.sum(np.abs(C1[ys, xs])))
            bound = G.budget_bound(C0[ys, xs].size, 21, nx, ny, scale, n_st, n_lv)
            print(f"{nx} x {ny} {what}: d sum(C) {d:.6e}, gauges {entered:.6e}, ends and walls {without:.6e}, "
                  f"|diff| {abs(d - entered - without):.3e}, bound {bound:.3e}")
            assert abs(d - (entered + without)) <= bound, what
            assert abs(d - without) > 1e3 * bound, what  # the gauges left out misses
        assert np.array_equal(got["right"][3], np.zeros(ny)) and np.array_equal(got["left"][3], np.zeros(ny))
    finally:
        A.close()


# ---- 5. lifecycle --------------------------------------------------------------------------------------------

def test_set_state_keeps_and_a_new_scalar_or_a_checkpoint_drops_the_gauges(gpu, tmp_path):
    nx, ny = LATTICES[0]
    ends, up, src, walls = cases(nx, ny)[NAMES[1]]
    ga = positions(nx, ny)
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        c0 = seeded_c0(nx, ny)
        set_all(A, c0, 3, ends, up, src, walls)
        A.set_scalar_gauges(**ga.kwargs())
        twin = Twin(B, c0, nx, ny, 3, ga, ends, up, src, walls)
        A.step(4)
        twin.run(S.pieces([4], 0, scalar=(0, 3)))
        assert_gauges_equal(A, ga, twin.sums, "before the new state")
        rho, u = W.perturbed_state(nx, ny, 8)
        A.set_state(rho, u)
        B.set_state(rho, u)
        assert_gauges_equal(A, ga, twin.sums, "at the new state")
        A.step(3)
        twin.run(S.pieces([3], 0, scalar=(0, 3)))
        assert_gauges_equal(A, ga, twin.sums, "the first event of the new state")
        assert_scalar_equal(A, twin.g, "the first event of the new state")
        assert twin.sums.substeps == 6
        # a replacement of the scalar drops the gauges, and so does its removal
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        assert A.scalar_gauges_info() == NONE_SET
        assert code_of(gpu, A.scalar_gauges) == L.IBLB_ERR_STATE
        g = S.equilibrium(c0, *velocity(B))
        A.step(3)
        B.step(3)
        assert_scalar_equal(A, S.event(g, *velocity(B), TAU, 3, walls), "the rule alone after the replacement")
        A.set_scalar_gauges(**ga.kwargs())
        assert A.scalar_gauges_info() == ga.info(0)
        A.remove_scalar()
        assert A.scalar_gauges_info() == NONE_SET
        assert code_of(gpu, lambda: A.set_scalar_gauges(**ga.kwargs())) == L.IBLB_ERR_STATE
        # a checkpoint holds neither
        set_all(A, c0, 3, ends, up, src, walls)
        A.set_scalar_gauges(**ga.kwargs())
        ck = str(tmp_path / "ck")
        A.save_checkpoint(ck)
        A.load_checkpoint(ck)
        assert A.scalar_gauges_info() == NONE_SET and A.scalar_info()["stride"] == 0
        A.step(5)
        B.step(5)
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 6. refusals leave everything as it was ------------------------------------------------------------------

def raw_set(A, n_stations, station, n_levels, level):
    """iblb_set_scalar_gauges with the struct as given: counts and arrays need not agree."""
    st = None if station is None else (C.c_int * max(len(station), 1))(*station)
    lv = None if level is None else (C.c_int * max(len(level), 1))(*level)
    ga = L.ScalarGauges(n_stations, None if st is None else C.addressof(st), n_levels,
                        None if lv is None else C.addressof(lv))
    return A._lib.iblb_set_scalar_gauges(A.handle, C.byref(ga))


def test_errors_leave_the_gauges_as_they_were(gpu):
    nx, ny = LATTICES[0]
    ends, up, src, walls = cases(nx, ny)[NAMES[0]]
    ga = positions(nx, ny)
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        # no scalar
        assert code_of(gpu, lambda: A.set_scalar_gauges(**ga.kwargs())) == L.IBLB_ERR_STATE
        assert A._lib.iblb_last_error(A.handle)
        assert code_of(gpu, A.remove_scalar_gauges) == L.IBLB_ERR_STATE
        assert A.scalar_gauges_info() == NONE_SET
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        # a scalar, no gauges
        assert code_of(gpu, A.scalar_gauges) == L.IBLB_ERR_STATE
        assert code_of(gpu, A.reset_scalar_gauges) == L.IBLB_ERR_STATE
        A.remove_scalar_gauges()  # nothing to remove: accepted, as iblb_set_scalar_ends(NULL) is
        st, lv = (C.c_int * 2)(-3, -4), (C.c_int * 2)(-5, -6)
        ns, nl, n = C.c_int(-1), C.c_int(-1), C.c_longlong(-1)
        assert A._lib.iblb_scalar_gauges_info(A.handle, C.byref(ns), st, C.byref(nl), lv, C.byref(n)) == L.IBLB_OK
        assert (ns.value, nl.value, n.value) == (0, 0, 0)
        assert list(st) == [-3, -4] and list(lv) == [-5, -6]  # none set: untouched
        A.set_scalar_gauges(**ga.kwargs())
        twin = Twin(B, c0, nx, ny, 3, ga, ends, up, src, walls)
        A.step(4)
        twin.run(S.pieces([4], 0, scalar=(0, 3)))
        info = A.scalar_gauges_info()
        assert info == ga.info(3)
        bad = {
            "both counts 0": (0, None, 0, None),
            "both counts 0, arrays given": (0, [1], 0, [1]),
            "a negative count of stations": (-1, [1], 1, [1]),
            "a negative count of levels": (1, [1], -2, [1]),
            "more stations than columns": (nx + 1, list(range(nx + 1)), 0, None),
            "more levels than links": (0, None, ny, list(range(ny))),
            "stations NULL, count 2": (2, None, 1, [1]),
            "levels NULL, count 1": (1, [1], 1, None),
            "a station at nx": (2, [0, nx], 0, None),
            "a negative station": (2, [-1, 3], 0, None),
            "stations repeated": (2, [3, 3], 0, None),
            "stations descending": (3, [2, 5, 4], 1, [1]),
            "a level at ny - 1": (1, [1], 2, [0, ny - 1]),
            "a negative level": (0, None, 1, [-1]),
            "levels repeated": (0, None, 2, [4, 4]),
            "levels descending beside good stations": (2, [0, nx - 1], 2, [5, 4]),
        }
        for name, args in bad.items():
            assert raw_set(A, *args) == L.IBLB_ERR_ARG, name
            assert A._lib.iblb_last_error(A.handle), name
            assert A.scalar_gauges_info() == info, name
            assert_gauges_equal(A, ga, twin.sums, name)
        with pytest.raises(gpu.IblbError):  # the same through the wrapper: a failed replacement
            A.set_scalar_gauges(stations=(4, 2), levels=(1,))
        assert_gauges_equal(A, ga, twin.sums, "the failed replacement")
        assert A._lib.iblb_get_scalar_gauges(A.handle, None, None, None, None, None) == L.IBLB_ERR_ARG
        # single outputs
        n = C.c_longlong(-1)
        assert A._lib.iblb_get_scalar_gauges(A.handle, None, None, None, None, C.byref(n)) == L.IBLB_OK and n.value == 3
        down = np.full((len(ga.levels), nx), -7.0)
        assert A._lib.iblb_get_scalar_gauges(A.handle, None, None, None, down.ctypes.data_as(C.c_void_p), None) == L.IBLB_OK
        assert np.array_equal(down, twin.sums.down)
        # the limits are accepted: every column a station, every link a level, and an array given with a count of 0
        assert raw_set(A, nx, list(range(nx)), ny - 1, list(range(ny - 1))) == L.IBLB_OK
        full = G.Gauges(range(nx), range(ny - 1))
        assert A.scalar_gauges_info() == full.info(0)
        assert raw_set(A, 1, [nx - 1], 0, [7]) == L.IBLB_OK
        assert A.scalar_gauges_info() == G.Gauges((nx - 1,), ()).info(0)
        keep = np.full(5, -7.0)  # a count of 0: its arrays are left untouched
        assert A._lib.iblb_get_scalar_gauges(A.handle, None, None, keep.ctypes.data_as(C.c_void_p), None, None) == L.IBLB_OK
        assert np.array_equal(keep, np.full(5, -7.0))
        # the scalar went on untouched by all of it: the next event (after iteration 6) with every gauge set
        assert raw_set(A, nx, list(range(nx)), ny - 1, list(range(ny - 1))) == L.IBLB_OK
        twin.gauges, twin.sums = full, G.Sums(full, nx, ny)
        A.step(2)
        twin.run([(2, {"scalar": True})])
        assert A.scalar_info()["updates"] == 2
        assert_scalar_equal(A, twin.g, "the next event")
        assert_gauges_equal(A, full, twin.sums, "the next event")
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
            assert raw_set(s, 1, [1], 1, [1]) == L.IBLB_ERR_STATE
            msg = s._lib.iblb_last_error(s.handle)
            assert msg and "group" in msg.decode()
            assert s._lib.iblb_reset_scalar_gauges(s.handle) == L.IBLB_ERR_STATE
            assert s.scalar_gauges_info() == NONE_SET
        assert all(np.array_equal(s.populations(), b) for s, b in zip(slabs, before))
        group.step(2)
        twin.step(2)
        for s, t in zip(slabs, twins):
            assert s.steps == t.steps == 4 and np.array_equal(s.populations(), t.populations())
            assert not np.array_equal(s.populations(), before[slabs.index(s)])
    finally:
        for s in slabs + twins:
            s.close()
