"""The scalar's fields IBLB_FIELD_C, _CUX, _CUY through every reader, and iblb_get_scalar_wall_flux, on the GPU
against tests/scalar_fields_ref.py (checked on the CPU by tests/test_scalar_fields_ref.py) applied to the same
lattice's scalar_populations() and fields(["ux", "uy"]): two readers the existing tests pin.

Lattices 20 x 18, 37 x 23 (an odd size, fewer rows than a wave) and 16 x 300 (more rows than the reduction's 256-row
workgroup, not a multiple of 64), f64 and f32 storage, tau 0.8, a seeded perturbed state and a body force with both
components, the seeded concentration of tests/test_gpu_scalar.py.

Values are compared with `==` (np.array_equal): C is the five stored populations added in the stated order, and the
products round once, which is what the numpy restatement does.  The sums of a reduction are within reduce_ref's
any-order bound.  The lattices carry no IB points (the spread's atomic order may differ in the last bits between two
contexts, tests/test_gpu_tracers.py).
"""
import ctypes as C
import math

import numpy as np
import pytest

import average_ref as AR
import reduce_ref as R
import scalar_fields_ref as F
import scalar_ref as S
import tracer_ref as T
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_average import ALL, assert_bins_equal, windows
from test_gpu_fields import BODY_FORCE
from test_gpu_reduce import blob
from test_gpu_scalar import seeded_c0
from test_gpu_tracers import new_lattice, point_set, seeds

pytestmark = pytest.mark.gpu

LATTICES = [(20, 18), (37, 23), (16, 300)]
PRECISIONS = ["f64", "f32"]
TAU = 0.8
NAMES = ["c", "cux", "cuy"]
BITS = [L.SCALAR_FIELDS[n] for n in NAMES]
VALUE_BELOW = ((S.VALUE, 0.25), (S.NOFLUX, 0.0))
WALLS = {
    "value / value": ((S.VALUE, 0.25), (S.VALUE, 1.75)),
    "value / no flux": VALUE_BELOW,
    "no flux / no flux": S.NO_FLUX_WALLS,
}
FLUID11 = [n for n in L.QUANTITIES if n not in L.SCALAR_FIELDS]
PATTERN = -7.0


def reference(lat):
    """c, cux, cuy of the whole lattice from its own populations and velocity, through the numpy restatement."""
    f = lat.fields(["ux", "uy"])
    return F.scalar_fields(lat.scalar_populations(), f["ux"], f["uy"])


def cut(a, w):
    if w is None:
        return a
    x0, y0, wnx, wny, sx, sy = w
    return a[y0:y0 + (wny - 1) * sy + 1:sy, x0:x0 + (wnx - 1) * sx + 1:sx]


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def code_of(gpu, call):
    with pytest.raises(gpu.IblbError) as e:
        call()
    return e.value.code


# ---- 1. fields ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_fields_equal_the_restatement(gpu, nx, ny, precision):
    """Before the first step, and after set_scalar(stride=2); step(5): the scalar is then one iteration behind the
    velocity it is multiplied with."""
    A = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=2, walls=VALUE_BELOW)
        for t in (0, 5):
            if t:
                A.step(t)
            assert A.steps == t and A.scalar_info()["updates"] == t // 2
            ref = reference(A)
            assert np.any(ref["cux"] != 0) and np.any(ref["cuy"] != 0)
            for name, w in windows(nx, ny).items():
                got = A.fields(NAMES, w)
                assert list(got) == NAMES, (t, name)
                for n in NAMES:
                    assert got[n].shape == cut(ref[n], w).shape, (t, name, n)
                    assert np.array_equal(got[n], cut(ref[n], w)), (t, name, n, np.max(np.abs(got[n] - cut(ref[n], w))))
                # mixed with the fluid's fields, given out of order: planes in ascending bit order
                mixed = A.fields(["cuy", "sxy", "rho", "c", "vort", "cux"], w)
                assert list(mixed) == ["rho", "vort", "sxy", "c", "cux", "cuy"], (t, name)
                old = A.fields(["rho", "vort", "sxy"], w)
                for n in mixed:
                    assert np.array_equal(mixed[n], old[n] if n in old else cut(ref[n], w)), (t, name, n)
                assert np.array_equal(A.fields("c", w)["c"], A.scalar(w)), (t, name)
                one = A.fields(["cuy"], w)
                assert list(one) == ["cuy"] and np.array_equal(one["cuy"], cut(ref["cuy"], w)), (t, name)
        # one iteration behind: C is that of the event after iteration 4, not a function of this state alone
        B = new_lattice(gpu, nx, ny, precision)
        try:
            B.step(5)
            assert np.array_equal(B.populations(), A.populations())
            B.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=2, walls=VALUE_BELOW)
            assert not np.array_equal(B.fields("c")["c"], A.fields("c")["c"])
        finally:
            B.close()
    finally:
        A.close()


# ---- 2. reduce ---------------------------------------------------------------------------------------------

def reduce_reference(lat, names, w):
    f = R.with_derived(lat.fields(ALL, w))
    f.update({n: cut(a, w) for n, a in reference(lat).items()})
    return R.reduce_ref({n: f[n] for n in sorted(names, key=L.QUANTITIES.get)}, 0)


def check_reduce(lat, names, w, what):
    ref = reduce_reference(lat, names, w)
    got = lat.reduce(names, w, rows=True, cols=True)
    assert list(got) == list(ref), what
    for n in got:
        R.check(got[n], ref[n], (what, n))
    return got


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_reduction_matches_the_reference(gpu, nx, ny, precision):
    A = new_lattice(gpu, nx, ny, precision)
    try:
        # a wall value far below the seed's [0, 1): the minimum moves to the wall's row, away from any seeded place
        walls = ((S.VALUE, -2.0), (S.NOFLUX, 0.0))
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=2, walls=walls)
        for t in (0, 5):
            if t:
                A.step(t)
            for name, w in windows(nx, ny).items():
                check_reduce(A, ["c"], w, (t, name, "c alone"))
                check_reduce(A, ["cuy", "c", "cux"], w, (t, name, "the three"))
                got = check_reduce(A, list(L.QUANTITIES), w, (t, name, "all fourteen"))
                n = nx * ny if w is None else w[2] * w[3]
                assert len(got) == 14 and all(s.count == n and s.nonfinite == 0 for s in got.values())
            bare = A.reduce("cux")
            R.check(bare["cux"], reduce_reference(A, ["cux"], None)["cux"], (t, "no sums"), rows=False, cols=False)
        whole = A.reduce("c")["c"]
        assert whole.min_j == 0 and whole.min < 0.0 <= seeded_c0(nx, ny).min() and whole.max > 0.5
        # one population of one cell not finite: counted in the scalar's three quantities and absent elsewhere
        g = A.scalar_populations()
        g[2, ny // 2, 3] = np.nan
        A.set_scalar(g0=g, tau=TAU, stride=2, walls=walls)
        got = check_reduce(A, list(L.QUANTITIES), None, "a NaN population")
        for n, s in got.items():
            assert (s.nonfinite, s.count) == ((1, nx * ny - 1) if n in NAMES else (0, nx * ny)), n
        assert np.isfinite([got[n].sum for n in NAMES]).all()
    finally:
        A.close()


# ---- 3. sample ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_samples_equal_the_reference(gpu, nx, ny, precision):
    """tracer_ref's special positions (the top row, the pair of columns across the x seam, the corners) and seeded
    points: the product is formed per cell, then interpolated."""
    A = new_lattice(gpu, nx, ny, precision)
    try:
        x, y = point_set(nx, ny, 200)
        spec = T.special_points(nx, ny)[0].size
        assert x.size == 200 > spec and np.any(y == ny - 1) and np.any(x > nx - 1)
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=2, walls=VALUE_BELOW)
        for t in (0, 5):
            if t:
                A.step(t)
            cells = reference(A)
            cells["ux"] = A.fields("ux")["ux"]
            for names in (NAMES, ["c"], ["cux", "ux", "c", "cuy"]):
                got = A.sample(names, x, y)
                assert list(got) == sorted(names, key=L.READ_FIELDS.get), (t, names)
                ref = T.sample_fields({n: cells[n] for n in got}, x, y)
                for n in got:
                    assert got[n].shape == (200,)
                    assert np.array_equal(got[n], ref[n]), (t, names, n, np.max(np.abs(got[n] - ref[n])))
            # not the interpolated C times the interpolated u
            both = A.sample(["c", "ux", "cux"], x, y)
            assert not np.array_equal(both["cux"], both["c"] * both["ux"])
            one = A.sample("cuy", x[8:9], y[8:9])
            assert np.array_equal(one["cuy"], T.sample(cells["cuy"], x[8:9], y[8:9]))
    finally:
        A.close()


# ---- 4. average --------------------------------------------------------------------------------------------

AVG = ["ux", "c", "cux", "cuy"]


@pytest.mark.parametrize("stride", [4, 6])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_averages_sample_the_scalar_after_its_event(gpu, nx, ny, precision, stride):
    """The scalar every 4 iterations, samples every `stride` (4: every sample shares its iteration with an event;
    6: the sample after iteration 12 does), tracers every 3, over step(9); step(11).  The twin B carries its own
    scalar and is stepped in the pieces the calls are cut into: after a piece its event has run, and its `fields`
    are the sample.  The bins built from C before the event differ.  D is A without the average."""
    A, B, D = (new_lattice(gpu, nx, ny, precision) for _ in range(3))
    try:
        c0 = seeded_c0(nx, ny)
        x0, y0 = seeds(nx, ny)
        for lat in (A, B, D):
            lat.set_scalar(c0, tau=TAU, stride=4, walls=VALUE_BELOW)
        for lat in (A, D):
            lat.set_tracers(x0, y0, stride=3)
        A.set_average(["cuy", "ux", "cux", "c"], stride=stride, nbins=2, squares=True)
        info = A.average_info()
        assert info["names"] == AVG and info["fields"] == 2 + 4096 + 8192 + 16384 and info["flags"] == L.AVG_SQ
        calls = [9, 11]
        plan = S.pieces(calls, 0, scalar=(0, 4), tracers=(0, 3), average=(0, stride))
        shared = [d["scalar"] for _, d in plan if d["average"]]
        assert shared == ([True] * 5 if stride == 4 else [False, True, False])
        for n in calls:
            A.step(n)
        after, before = [], []
        for n, due in plan:
            g_prev = B.scalar_populations()
            B.step(n)
            D.step(n)
            if due["average"]:
                f = B.fields(AVG)
                after.append({k: v.copy() for k, v in f.items()})
                old = F.scalar_fields(g_prev, f["ux"], B.fields("uy")["uy"])
                before.append({"ux": f["ux"].copy(), **old})
        assert B.scalar_info()["updates"] == A.scalar_info()["updates"] == 5
        ref = AR.accumulate(after, 2, squares=True)
        assert_bins_equal(A, ref, f"stride {stride}")
        assert A.average_info()["samples_total"] == len(after) == 20 // stride
        wrong = AR.accumulate(before, 2, squares=True)
        differs = [b for b in range(2) for n in NAMES if not np.array_equal(wrong[b]["sum"][n], ref[b]["sum"][n])]
        assert differs, "the order of the event and the sample is untested"
        assert np.array_equal(A.mean(0)["c"], ref[0]["sum"]["c"] / float(ref[0]["samples"]))
        # the average changes nothing else
        for a, d in zip(A.tracers(), D.tracers()):
            assert np.array_equal(a, d)
        assert np.array_equal(A.populations(), D.populations()) and np.array_equal(A.populations(), B.populations())
        assert np.array_equal(A.scalar_populations(), D.scalar_populations())
        assert np.array_equal(A.scalar_populations(), B.scalar_populations())
    finally:
        for lat in (A, B, D):
            lat.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_averages_on_windows(gpu, nx, ny, precision):
    A = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=3, walls=VALUE_BELOW)
        for name, w in windows(nx, ny).items():
            A.set_average(NAMES + ["sxy"], window=w, stride=3, squares=True)  # replaces the previous set
            samples = []
            for _ in range(2):
                A.step(3)
                samples.append({k: v.copy() for k, v in A.fields(["sxy"] + NAMES, w).items()})
            assert_bins_equal(A, AR.accumulate(samples, 1, squares=True), name)
    finally:
        A.close()


# ---- 5. wall flux ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("walls", list(WALLS))
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_wall_flux(gpu, nx, ny, precision, walls, stride):
    A = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=stride, walls=WALLS[walls])
        A.step(3)
        assert A.scalar_info()["updates"] == 3 // stride

        def check(what):
            bottom, top = A.scalar_wall_flux()
            g = A.scalar_populations()
            rb, rt = F.wall_flux(g, WALLS[walls])
            assert bottom.shape == top.shape == (nx,)
            assert np.array_equal(bottom, rb) and np.array_equal(top, rt), what
            for (kind, _), side in zip(WALLS[walls], (bottom, top)):
                if kind == S.NOFLUX:
                    assert np.all(side == 0.0) and not np.any(np.signbit(side)), what
                else:
                    assert np.all(side != 0.0), what
            return bottom, top, g

        check("after step(3)")
        # either side alone
        lib, h = A._lib, A.handle
        one = np.full(nx, PATTERN)
        assert lib.iblb_get_scalar_wall_flux(h, None, p(one)) == L.IBLB_OK
        assert np.array_equal(one, F.wall_flux(A.scalar_populations(), WALLS[walls])[1])
        if stride == 1:
            # the budget of one substep: what entered through the walls is the change of sum(C)
            s0 = A.reduce("c")["c"].sum
            A.step(1)
            bottom, top, g = check("after one more substep")
            s1 = A.reduce("c")["c"].sum
            flux = math.fsum(np.concatenate([bottom, top]))
            bound = 4 * nx * ny * 2.0 ** -53 * math.fsum(np.abs(g).ravel())
            print(f"{nx}x{ny} {precision} {walls}: flux {flux:.17g} change {s1 - s0:.17g} "
                  f"|diff| {abs(flux - (s1 - s0)):.3e} bound {bound:.3e}")
            assert abs(flux - (s1 - s0)) <= bound
            assert (abs(flux) > 1e3 * bound) == (walls != "no flux / no flux")
    finally:
        A.close()


# ---- 6. states and refusals ----------------------------------------------------------------------------------

def raw_calls(A, nx, ny):
    """The four entry points on lattice A with outputs prefilled with a pattern: {name: (call(bits) -> rc, untouched())}."""
    lib, h = A._lib, A.handle
    out = np.full(3 * nx * ny, PATTERN)
    st = (L.FieldStats * 3)()
    C.memset(st, 0x5A, C.sizeof(st))
    st0 = bytes(st)
    rs, cs = np.full(3 * ny, PATTERN), np.full(3 * nx, PATTERN)
    px, py = np.array([0.5, 3.25, nx - 0.5]), np.array([0.5, 2.0, ny - 1.0])
    so = np.full(9, PATTERN)
    return {
        "iblb_get_fields": (lambda b: lib.iblb_get_fields(h, None, b, p(out)), lambda: np.all(out == PATTERN)),
        "iblb_reduce_fields": (lambda b: lib.iblb_reduce_fields(h, None, b, st, p(rs), p(cs)),
                               lambda: bytes(st) == st0 and np.all(rs == PATTERN) and np.all(cs == PATTERN)),
        "iblb_sample_points": (lambda b: lib.iblb_sample_points(h, 3, p(px), p(py), b, p(so)), lambda: np.all(so == PATTERN)),
        "iblb_set_average": (lambda b: lib.iblb_set_average(h, None, b, 2, 1, 0), lambda: True),
    }


def test_a_scalar_bit_without_a_scalar_is_a_state_error(gpu):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        A.step(2)
        A.set_average(["ux"], stride=3)
        info = A.average_info()
        for name, (call, untouched) in raw_calls(A, nx, ny).items():
            for bits in BITS + [sum(BITS), 4096 | 2, 8192 | 64 | 8]:
                assert call(bits) == L.IBLB_ERR_STATE, (name, bits)
                assert A._lib.iblb_last_error(A.handle), (name, bits)
                assert untouched(), (name, bits)
            assert A.average_info() == info, name
        # the argument errors come first, with the messages they had
        lib, h = A._lib, A.handle
        bad = L.Window(nx - 2, 0, 2, 2, 2, 1)
        out = np.full(nx * ny, PATTERN)
        assert lib.iblb_get_fields(h, C.byref(bad), 4096, p(out)) == L.IBLB_ERR_ARG
        assert lib.iblb_get_fields(h, None, 4096, None) == L.IBLB_ERR_ARG
        assert lib.iblb_set_average(h, None, 4096, 0, 1, 0) == L.IBLB_ERR_ARG
        assert lib.iblb_set_average(h, None, 4096, 1, 1, 4) == L.IBLB_ERR_ARG
        px, py = np.array([float(nx)]), np.array([0.0])
        assert lib.iblb_sample_points(h, 1, p(px), p(py), 4096, p(out)) == L.IBLB_ERR_ARG
        # the wall flux
        b, t = np.full(nx, PATTERN), np.full(nx, PATTERN)
        assert lib.iblb_get_scalar_wall_flux(h, p(b), p(t)) == L.IBLB_ERR_STATE
        assert np.all(b == PATTERN) and np.all(t == PATTERN)
        assert code_of(gpu, lambda: A.fields("c")) == code_of(gpu, lambda: A.reduce("cux")) == L.IBLB_ERR_STATE
        assert code_of(gpu, lambda: A.sample("cuy", [1.0], [1.0])) == L.IBLB_ERR_STATE
        assert code_of(gpu, lambda: A.set_average(["c"])) == code_of(gpu, A.scalar_wall_flux) == L.IBLB_ERR_STATE
        assert A.average_info() == info
        # the previous average goes on as it was: set after iteration 2, its first sample after iteration 5
        A.step(3)
        assert A.average_info()["samples_total"] == 1
        assert np.array_equal(A.average(0)["sum"]["ux"], A.fields("ux")["ux"])
        with pytest.raises(ValueError):
            A.fields("momx")
        with pytest.raises(ValueError):
            A.set_average(["usq"])
    finally:
        A.close()


def test_unknown_bits_stay_unknown(gpu):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        for with_scalar in (False, True):
            if with_scalar:
                A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=2)
            for name, (call, untouched) in raw_calls(A, nx, ny).items():
                for bits in (2048, 2048 | 4096, 2048 | 1, 32768, 1 << 31):
                    assert call(bits) == L.IBLB_ERR_ARG, (with_scalar, name, bits)
                    assert untouched(), (with_scalar, name, bits)
                # 128 .. 1024 stay the reduction's own
                for bits in (128, 256, 512, 1024, 128 | 4096):
                    want = L.IBLB_ERR_ARG if name != "iblb_reduce_fields" else (
                        L.IBLB_OK if with_scalar or not bits & 4096 else L.IBLB_ERR_STATE)
                    assert call(bits) == want, (with_scalar, name, bits)
            assert A.average_info()["fields"] == 0
    finally:
        A.close()


def test_the_scalar_stays_while_an_average_samples_it(gpu, tmp_path):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        lib, h = A._lib, A.handle
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=2, walls=VALUE_BELOW)
        assert lib.iblb_get_scalar_wall_flux(h, None, None) == L.IBLB_ERR_ARG and lib.iblb_last_error(h)
        A.set_average(["c", "ux"], stride=2)
        A.step(2)
        sinfo, ainfo, g, acc = A.scalar_info(), A.average_info(), A.scalar_populations(), A.average(0)
        assert ainfo["samples_total"] == 1 and np.array_equal(acc["sum"]["c"], S.concentration(g))
        # removing the scalar under the average: refused, nothing changed
        assert code_of(gpu, A.remove_scalar) == L.IBLB_ERR_STATE
        assert lib.iblb_last_error(h)
        assert A.scalar_info() == sinfo and A.average_info() == ainfo
        assert np.array_equal(A.scalar_populations(), g)
        assert np.array_equal(A.average(0)["sum"]["c"], acc["sum"]["c"])
        # replacing it is allowed, and the average goes on with the new one
        c1 = 2.0 + c0
        A.set_scalar(c1, tau=0.9, stride=2)
        assert A.average_info() == ainfo
        A.step(2)
        assert A.average_info()["samples_total"] == 2 and A.scalar_info()["updates"] == 1
        now = A.fields("c")["c"]
        assert np.min(now) > 1.5 and np.array_equal(A.average(0)["sum"]["c"], acc["sum"]["c"] + now)
        # an average without a scalar bit does not hold the scalar
        A.set_average(["ux"], stride=2)
        A.remove_scalar()
        assert A.scalar_info()["stride"] == 0
        # after removing the average, removal of the scalar succeeds
        A.set_scalar(c0, tau=TAU, stride=2)
        A.set_average(["cux"], stride=2)
        assert code_of(gpu, A.remove_scalar) == L.IBLB_ERR_STATE
        A.set_average([])
        A.remove_scalar()
        assert A.scalar_info()["stride"] == 0 and A.average_info()["fields"] == 0
        # a checkpoint leaves neither
        A.set_scalar(c0, tau=TAU, stride=2)
        A.set_average(["c"], stride=2)
        ck = str(tmp_path / "ck")
        A.save_checkpoint(ck)
        A.load_checkpoint(ck)
        assert A.scalar_info()["stride"] == 0 and A.average_info()["fields"] == 0
        assert code_of(gpu, lambda: A.fields("c")) == L.IBLB_ERR_STATE
        A.step(4)
    finally:
        A.close()


def test_a_slab_of_a_group_holds_no_scalar(gpu):
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
            for n in NAMES:
                assert code_of(gpu, lambda: s.fields(n)) == L.IBLB_ERR_STATE, n
                assert code_of(gpu, lambda: s.reduce(["rho", n], rows=True)) == L.IBLB_ERR_STATE, n
                assert s._lib.iblb_last_error(s.handle)
        assert code_of(gpu, lambda: group.fields(NAMES)) == L.IBLB_ERR_STATE
        assert code_of(gpu, lambda: group.reduce("c")) == L.IBLB_ERR_STATE
        # the vorticity refusal still comes first
        assert code_of(gpu, lambda: slabs[0].fields(["vort", "c"])) == L.IBLB_ERR_UNSUPPORTED
        group.step(2)
        assert group.fields("ux")["ux"].shape == (ny, nx)
    finally:
        for s in slabs:
            s.close()


# ---- 7. the old path -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES[1:])
def test_without_a_scalar_bit_the_readers_are_what_they_were(gpu, nx, ny, precision):
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_scalar(seeded_c0(nx, ny), tau=TAU, stride=5)
        for lat in (A, B):
            lat.set_average(ALL, stride=5, nbins=2, squares=True, uxuy=True)
            lat.step(5)
            lat.step(5)
        assert A.scalar_info()["updates"] == 2
        fa, fb = A.fields(ALL), B.fields(ALL)
        assert list(fa) == list(fb) == ALL and all(np.array_equal(fa[n], fb[n]) for n in ALL)
        assert blob(A.reduce(FLUID11, rows=True, cols=True)) == blob(B.reduce(FLUID11, rows=True, cols=True))
        assert len(FLUID11) == 11
        x, y = point_set(nx, ny, 100)
        sa, sb = A.sample(ALL, x, y), B.sample(ALL, x, y)
        assert all(np.array_equal(sa[n], sb[n]) for n in ALL)
        for b in range(2):
            ga, gb = A.average(b), B.average(b)
            assert ga["samples"] == gb["samples"] == 1 and np.array_equal(ga["sum_uxuy"], gb["sum_uxuy"])
            for n in ALL:
                assert np.array_equal(ga["sum"][n], gb["sum"][n]) and np.array_equal(ga["sum_sq"][n], gb["sum_sq"][n])
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
        A.set_average(["c"], stride=7)
        ta, tb = A.timing(), B.timing()
        A.step(14)
        B.step(7)
        B.step(7)
        ta1, tb1 = A.timing(), B.timing()
        for k in ("deep_launches", "deep_iterations"):
            assert ta1[k] - ta[k] == tb1[k] - tb[k], (k, ta[k], ta1[k], tb[k], tb1[k])
        assert tb1["deep_launches"] - tb["deep_launches"] > 0
        assert A.scalar_info()["updates"] == 2 and A.average_info()["samples_total"] == 2
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()
