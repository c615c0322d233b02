"""Every build of the passive scalar's substep on the GPU against its twin, edges included: the 16 combinations of a
source, an uptake, open ends and gauges (the compile-time switches of scalar_push, csrc/scalar_kernels.hip), each built
as scalar_first_kernel<double>, scalar_first_kernel<float> and scalar_next_kernel: 48 kernels, chosen at the launch by
which device arrays are set.  The cases are those of tests/scalar_matrix.py, pinned on the CPU by
tests/test_scalar_matrix.py: in each, every switched-on feature and every slot of a pair changes what the restatement
returns, so a build that read wall_value[0] for [1], row 2 of the source's walls for row 3 or kind[0] for kind[1] fails
here.

Lattices.  1 x 2 and 5 x 257 run all 16 combinations under all four pairs of wall kinds; 2 x 3 and 33 x 70 run the 16
combinations with the wall pair rotated by the combination's index.  1 x 2: a column is its own left and right
neighbour, one lane writes both ends' entries, the two wall rows are adjacent and there is a single level.  2 x 3: both
x-neighbours are the same column.  33 x 70: one column past the 32-wide transpose tile, six rows past a wave.  5 x 257:
the top wall row sits alone in the second workgroup, and the level 255 has its two writers in different workgroups.
Both precisions: 2 x (2 x 64 + 2 x 16) = 320 cases, each two lattices of thirteen iterations.

Every comparison is `==` (np.array_equal), the scalar's contract: one rounding per operation, one writer per entry,
no atomics, and no IB points on the twins.  The twin's velocity is Lattice.fields(["ux", "uy"]), which the last test
pins at the narrow sizes against tests/fields_ref.py with the bounds of tests/test_gpu_fields.py.
"""
import numpy as np
import pytest

import fields_ref as R
import scalar_matrix as M
import scalar_ref as S
import scalar_source_ref as Q
import scalar_uptake_ref as U
import scalar_ends_ref as E
import scalar_gauges_ref as G
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_fields import ALL, check
from test_gpu_scalar import PRECISIONS, TAU, seeded_c0, velocity
from test_gpu_scalar import assert_scalar_equal
from test_gpu_scalar_ends import NONE_SET as ENDS_NONE_SET
from test_gpu_scalar_ends import assert_sums_equal, code_of, info_of
from test_gpu_scalar_gauges import NONE_SET, Twin, assert_gauges_equal
from test_gpu_tracers import new_lattice

pytestmark = pytest.mark.gpu

SOURCE_NONE_SET = {"decay": 0.0, "present": 0}
UPTAKE_NONE_SET = {"present": 0, "substeps": 0}


def assert_all_equal(gpu, A, twin, what):
    """The populations and C, the sums of every family that is set, every *_info (so the combination in force is the
    one meant: these are what choose the build), the getters' refusal of what is not set, and the wall flux reader."""
    assert_scalar_equal(A, twin.g, what)
    src, up, ends, ga = twin.src, twin.up, twin.ends, twin.gauges
    if src is None:
        assert A.scalar_source_info() == SOURCE_NONE_SET, what
        assert code_of(gpu, A.scalar_source) == L.IBLB_ERR_STATE, what
    else:
        assert A.scalar_source_info() == {"decay": src.decay, "present": src.present()}, what
        assert np.array_equal(A.scalar_source(), src.source), what
    if up is None:
        assert A.scalar_uptake_info() == UPTAKE_NONE_SET, what
        assert code_of(gpu, A.scalar_uptake) == L.IBLB_ERR_STATE, what
    else:
        assert_sums_equal(A.scalar_uptake(), twin.us, (what, "uptake"))
        assert A.scalar_uptake_info() == {"present": up.present(), "substeps": twin.us.substeps}, what
    if ends is None:
        assert A.scalar_ends_info() == ENDS_NONE_SET, what
        assert code_of(gpu, A.scalar_ends) == L.IBLB_ERR_STATE, what
    else:
        assert_sums_equal(A.scalar_ends(), twin.es, (what, "ends"))
        assert A.scalar_ends_info() == info_of(ends, twin.es.substeps), what
    if ga is None:
        assert A.scalar_gauges_info() == NONE_SET, what
        assert code_of(gpu, A.scalar_gauges) == L.IBLB_ERR_STATE, what
    else:
        assert_gauges_equal(A, ga, twin.sums, what)
    for k, (got, want) in enumerate(zip(A.scalar_wall_flux(),
                                        Q.wall_flux(twin.g, src if src is not None else Q.Source(), twin.walls))):
        assert np.array_equal(got, want), (what, "wall flux", k)


SETTERS = {
    "source": lambda A, v: A.set_scalar_source(**v.kwargs()),
    "uptake": lambda A, v: A.set_scalar_uptake(**v.kwargs()),
    "ends": lambda A, v: A.set_scalar_ends(**v.kwargs()),
    "gauges": lambda A, v: A.set_scalar_gauges(**v.kwargs()),
}
REMOVERS = {"source": "remove_scalar_source", "uptake": "remove_scalar_uptake", "ends": "remove_scalar_ends",
            "gauges": "remove_scalar_gauges"}


def twin_set(twin, name, v):
    """The twin's side of one iblb_set_scalar_* (v None: the removal): the feature's own sums start at zero, the
    others' carry on."""
    nx, ny = twin.nx, twin.ny
    if name == "source":
        twin.src = v
    elif name == "uptake":
        twin.up, twin.us = v, None if v is None else U.Sums(nx)
    elif name == "ends":
        twin.ends, twin.es = v, None if v is None else E.Sums(ny)
    else:
        twin.gauges, twin.sums = v, None if v is None else G.Sums(v, nx, ny)


# ---- a. every build equals the twin ----------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny,ci,walls_name", M.matrix(), ids=[M.case_id(*c) for c in M.matrix()])
def test_every_build_equals_the_twin(gpu, nx, ny, ci, walls_name, precision):
    """step(2), the scalar set with stride 3, the case's features set, step(5), step(6): the events fall at the
    iterations 5, 8 and 11, inside the calls and across them, and each runs one first substep and two next ones."""
    ends, up, src, ga, walls = M.case(nx, ny, M.COMBOS[ci], walls_name)
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        B.step(2)
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=3, walls=walls)
        for name, v in (("source", src), ("uptake", up), ("ends", ends), ("gauges", ga)):
            if v is not None:
                SETTERS[name](A, v)
        info = A.scalar_info()
        assert (info["tau"], info["stride"], info["updates"]) == (TAU, 3, 0)
        assert info["walls"] == tuple((k, float(v)) for k, v in walls)
        twin = Twin(B, c0, nx, ny, 3, ga, ends, up, src, walls)
        assert_all_equal(gpu, A, twin, "at the set")
        t = 2
        for n, events in ((5, 1), (6, 2)):
            plan = S.pieces([n], t, scalar=(2, 3))
            assert sum(1 for _, d in plan if d["scalar"]) == events
            A.step(n)
            twin.run(plan)
            t += n
            assert_all_equal(gpu, A, twin, f"after iteration {t}")
        assert A.scalar_info()["updates"] == 3
        for sums in (twin.sums, twin.es, twin.us):
            assert sums is None or sums.substeps == 9
        assert A.steps == B.steps == 13 and np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- b. the four features set and removed in any order --------------------------------------------------------

@pytest.mark.parametrize("order", M.orders(), ids=["-".join(o) for o in M.orders()])
def test_features_set_in_any_order(gpu, order):
    """33 x 70, f64, stride 2, no flux below and value 0.4 above.  The four features set one at a time in `order`, one
    event after each; then removed one at a time, the order reversed and rotated by two (no feature leaves at the
    place it came), one event after each.  Every iblb_set_scalar_* keeps the other three and their totals, and what
    is removed is refused by its getter."""
    nx, ny = 33, 70
    walls_name = "no flux / value 0.4"
    ends, up, src, ga, walls = M.case(nx, ny, (True, True, True, True), walls_name)
    values = {"source": src, "uptake": up, "ends": ends, "gauges": ga}
    removal = order[::-1][2:] + order[::-1][:2]
    assert sorted(removal) == sorted(order) and all(a != b for a, b in zip(order, removal))
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=2, walls=walls)
        twin = Twin(B, c0, nx, ny, 2, None, None, None, None, walls)
        events = 0

        def event(what):
            nonlocal events
            A.step(2)
            B.step(2)
            twin.event()
            events += 1
            assert A.scalar_info()["updates"] == events, what
            assert_all_equal(gpu, A, twin, what)

        for name in order:
            SETTERS[name](A, values[name])
            twin_set(twin, name, values[name])
            assert_all_equal(gpu, A, twin, f"at the set of the {name}")
            event(f"the event after the set of the {name}")
        # every family has run since its own set: 2 substeps per event
        assert {n: s.substeps for n, s in (("uptake", twin.us), ("ends", twin.es), ("gauges", twin.sums))} == \
            {n: 2 * (4 - order.index(n)) for n in ("uptake", "ends", "gauges")}
        for name in removal:
            getattr(A, REMOVERS[name])()
            twin_set(twin, name, None)
            assert_all_equal(gpu, A, twin, f"at the removal of the {name}")
            event(f"the event after the removal of the {name}")
        assert events == 8 and A.steps == B.steps == 16 and np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- c. the twin's input on the narrow lattices ---------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", [(1, 2), (2, 3), (5, 257)])
def test_fields_on_narrow_lattices_feed_the_twin_correctly(gpu, nx, ny, precision):
    """Lattice.fields against tests/fields_ref.py applied to the same lattice's macro() and populations(), as
    tests/test_gpu_fields.py does and with its bounds, at the iterations the matrix reads the velocity (and before the
    first step): the velocity the twins take is the one iblb_get_macro returns, bit for bit."""
    lat = new_lattice(gpu, nx, ny, precision)
    try:
        done = 0
        for t in (0, 2, 5, 8, 11):
            if t > done:
                lat.step(t - done)
            done = t
            rho, u = lat.macro()
            ref = R.fields_ref(rho, u, lat.populations(), W.TAU, nx, ny)
            check(lat.fields(ALL), ref, rho, u, ALL, (nx, ny, precision, t))
            ux, uy = velocity(lat)
            assert ux.shape == uy.shape == (ny, nx)
            assert np.array_equal(ux, ref["ux"]) and np.array_equal(uy, ref["uy"]), t
            assert np.all(np.isfinite(ux)) and np.any(ux != 0.0) and np.any(uy != 0.0), t
    finally:
        lat.close()
