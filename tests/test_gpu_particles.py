"""The tracers under a motion model (iblb_set_tracer_model) on the GPU against tests/particle_ref.py (checked on
the CPU by tests/test_particle_ref.py) applied to what Lattice.fields returns for the same state.

Lattices 20 x 18 and 37 x 23, f64 and f32 storage, the seeded perturbed state and the body force of
tests/test_gpu_tracers.py.  Positions, laps, statuses and hit iterations are compared with `==`: the device samples
the velocity with the functions of the plain tracers, hashes in 64-bit integers and does one rounding per operation,
and the host twin is stepped in exactly the pieces iblb_step cuts its calls into.  A twin's velocity fields at the
update iterations are computed once per (lattice, precision, schedule) and shared.  The twins of the `==` comparisons
carry no IB points: with moving IB points the spread's atomic order may differ in the last bits between two contexts
and a fate can flip on them, so there only invariants are checked.
"""
import ctypes as C

import numpy as np
import pytest

import particle_ref as P
import tracer_ref as T
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_tracers import LATTICES, PRECISIONS, COUNTS, moving_points, new_lattice, pieces, point_set

pytestmark = pytest.mark.gpu

KINDS = ["clamp", "reflect", "absorb"]
DRIFT = (0.003, -0.002)
D = 0.05
UPDATES = {1: 60, 3: 40, 8: 15}  # per stride: 2 D stride updates = 6, 12, 12 rows^2 of spreading


def seeds(nx, ny, n=1000):
    """n tracers: the special positions of tracer_ref, cell centres, six on each wall's row, then random ones."""
    x, y = point_set(nx, ny, max(n, 66), seed=5)
    y[54:60], y[60:66] = 0.0, ny - 1.0
    return x[:n].copy(), y[:n].copy()


def model(walls=("absorb", "reflect"), diffusivity=D, drift=DRIFT, seed=2024):
    return dict(diffusivity=diffusivity, drift=drift, walls=walls, seed=seed)


def ref_model(m):
    return dict(diffusivity=m["diffusivity"], drift=m["drift"], walls=tuple(P.WALLS[w] for w in m["walls"]), seed=m["seed"])


_TWINS = {}


def twin_fields(gpu, nx, ny, precision, stride, calls, t0=0, state_seed=7):
    """[(iteration, ux, uy)] at the update iterations of tracers set at t0 and stepped by `calls`, from a twin
    lattice stepped in the pieces iblb_step cuts the calls into; computed once and shared, never written to."""
    key = (nx, ny, precision, stride, tuple(calls), t0, state_seed)
    if key not in _TWINS:
        B = new_lattice(gpu, nx, ny, precision, state=W.perturbed_state(nx, ny, state_seed))
        try:
            out = []
            if t0:
                B.step(t0)
            for n, update in pieces(t0, stride, t0, calls):
                B.step(n)
                if update:
                    f = B.fields(["ux", "uy"])
                    for a in f.values():
                        a.setflags(write=False)
                    out.append((B.steps, f["ux"], f["uy"]))
            _TWINS[key] = out
        finally:
            B.close()
    return _TWINS[key]


def fresh(x, y):
    n = x.size
    return x, y, np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int64)


def reference(fields, state, stride, m, m0=0, t_of=lambda t: t):
    """The state (x, y, laps, status, hit) after the updates of `fields`, the first one update number m0; also the
    number of reflections."""
    x, y, laps, st, hit = state
    k = ref_model(m)
    reflected = 0
    for i, (t, ux, uy) in enumerate(fields):
        x, y, laps, st, hit, r = P.advect(ux, uy, x, y, laps, st, hit, stride, m0 + i, t_of(t), **k)
        reflected += int(r.sum())
    return (x, y, laps, st, hit), reflected


def device_state(A):
    x, y, laps = A.tracers()
    st, hit = A.tracer_fates()
    return x, y, laps, st, hit


def assert_same(got, want, what=""):
    for name, g, w in zip(("x", "y", "laps", "status", "hit"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, int(np.sum(g != w)))


def assert_in_range(x, y, nx, ny):
    assert np.all(np.isfinite(x) & np.isfinite(y))
    assert np.all((x >= 0) & (x < nx) & (y >= 0) & (y <= ny - 1))


def assert_something_happened(state0, state, reflected, walls, nx, ny):
    """On the reference's own result: a test cannot pass because nothing happened."""
    x, y, laps, st, hit = state
    n = x.size
    for w, s in enumerate((P.AT_BOTTOM, P.AT_TOP)):
        if walls[w] == "absorb":
            assert np.sum(st == s) >= 0.03 * n, (w, int(np.sum(st == s)))
            assert np.all(y[st == s] == (0.0, ny - 1.0)[w]) and np.all(hit[st == s] > 0)
        else:
            assert not np.any(st == s)
    assert np.sum(st == P.ALIVE) >= 0.25 * n and np.all(hit[st == P.ALIVE] == -1)
    assert np.any(laps != 0)
    if "reflect" in walls:
        assert reflected >= 1
    assert_in_range(x, y, nx, ny)


# ---- the update rule ----------------------------------------------------------------------------------

def run_against_reference(gpu, nx, ny, precision, stride, walls, n=1000, check=True):
    m = model(walls)
    total = stride * UPDATES[stride]
    fields = twin_fields(gpu, nx, ny, precision, stride, [total])
    assert len(fields) == UPDATES[stride]
    x0, y0 = seeds(nx, ny, n)
    want, reflected = reference(fields, fresh(x0, y0), stride, m)
    if check:
        assert_something_happened(fresh(x0, y0), want, reflected, walls, nx, ny)
    A = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_tracers(x0, y0, stride=stride)
        A.set_tracer_model(**m)
        info = A.tracer_model_info()
        assert info == {"present": True, "diffusivity": D, "drift": DRIFT, "walls": tuple(walls), "seed": 2024,
                        "alive": n, "at_bottom": 0, "at_top": 0}
        A.step(total)  # one long call
        assert A.tracer_info() == {"n": n, "stride": stride, "updates": UPDATES[stride]}
        assert_same(device_state(A), want, (nx, ny, precision, stride, walls))
        info = A.tracer_model_info()
        st = want[3]
        assert (info["alive"], info["at_bottom"], info["at_top"]) == tuple(int(np.sum(st == s)) for s in (0, 1, 2))
    finally:
        A.close()


@pytest.mark.parametrize("top", KINDS)
@pytest.mark.parametrize("bottom", KINDS)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_every_pair_of_walls_equals_the_reference(gpu, nx, ny, precision, bottom, top):
    run_against_reference(gpu, nx, ny, precision, 3, (bottom, top))


@pytest.mark.parametrize("stride", [1, 8])  # 8: a deep sweep between updates
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_the_other_strides_equal_the_reference(gpu, nx, ny, precision, stride):
    run_against_reference(gpu, nx, ny, precision, stride, ("absorb", "reflect"))
    run_against_reference(gpu, nx, ny, precision, stride, ("reflect", "absorb"))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_tracer_count_equals_the_reference(gpu, precision, n):
    nx, ny = LATTICES[1]
    run_against_reference(gpu, nx, ny, precision, 3, ("absorb", "absorb"), n=n, check=n == 1000)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_updates_count_on_across_calls(gpu, nx, ny, precision):
    """step(3); step(4); step(13); step(100) at stride 5 with tracers set at t0 = 2: the updates fall inside the
    calls, and the random numbers go by the update count."""
    stride, calls, walls = 5, [3, 4, 13, 100], ("absorb", "reflect")
    m = model(walls)
    fields = twin_fields(gpu, nx, ny, precision, stride, calls, t0=2)
    assert [t for t, _, _ in fields] == list(range(7, 123, 5))
    x0, y0 = seeds(nx, ny)
    want, reflected = reference(fields, fresh(x0, y0), stride, m)
    assert_something_happened(fresh(x0, y0), want, reflected, walls, nx, ny)
    A = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        A.set_tracers(x0, y0, stride=stride)
        A.set_tracer_model(**m)
        for k, n in enumerate(calls):
            A.step(n)
            if k == 1:  # after step(3), step(4): one update, after iteration 7
                one, _ = reference(fields[:1], fresh(x0, y0), stride, m)
                assert A.tracer_info()["updates"] == 1
                assert_same(device_state(A), one, "after the first update")
        assert A.tracer_info()["updates"] == len(fields) and A.steps == 122
        assert_same(device_state(A), want)
    finally:
        A.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_the_zero_model_is_the_plain_tracers(gpu, nx, ny, precision):
    from test_gpu_tracers import edge_seeds, fast_state
    for state, (x0, y0), steps in ((fast_state(nx, ny), edge_seeds(nx, ny), 4), (None, seeds(nx, ny, 300), 12)):
        A = new_lattice(gpu, nx, ny, precision, state=state)
        B = new_lattice(gpu, nx, ny, precision, state=state)
        try:
            A.set_tracers(x0, y0, stride=1)
            A.set_tracer_model(seed=77)
            B.set_tracers(x0, y0, stride=1)
            A.step(steps)
            B.step(steps)
            (ax, ay, al), (bx, by, bl) = A.tracers(), B.tracers()
            assert np.array_equal(ax, bx) and np.array_equal(ay, by) and np.array_equal(al, bl)
            assert not np.array_equal(ax, x0)
            if state is not None:  # the case is not empty: wraps both ways and clamps at both walls
                assert np.any(bl > 0) and np.any(bl < 0)
                assert np.any((by == 0.0) & (y0 > 0.0)) and np.any((by == ny - 1.0) & (y0 < ny - 1.0))
            st, hit = A.tracer_fates()
            assert not st.any() and np.all(hit == -1)
            assert A.tracer_model_info()["alive"] == x0.size
            assert np.array_equal(A.populations(), B.populations())
        finally:
            A.close()
            B.close()


# ---- edges --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("walls", [("absorb", "absorb"), ("reflect", "reflect"), ("clamp", "absorb")])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_special_positions_and_wall_rows(gpu, nx, ny, precision, walls):
    """The special positions of tracer_ref and tracers on both walls' rows, each twice, under a drift towards
    either wall: a start on the wall's row deposits where it is (lam = 0) or is folded back."""
    sx, sy = T.special_points(nx, ny)
    cols = np.arange(0.5, nx, 2.25)
    x0 = np.concatenate([sx, cols, cols])
    y0 = np.concatenate([sy, np.zeros(cols.size), np.full(cols.size, ny - 1.0)])
    fields = twin_fields(gpu, nx, ny, precision, 3, [9])
    for drift_y in (-0.05, 0.05):
        m = model(walls, diffusivity=0.0001, drift=(0.01, drift_y))  # amp = 0.042 against a drift of 0.15 an update
        want, _ = reference(fields, fresh(x0, y0), 3, m)
        row = 0.0 if drift_y < 0 else ny - 1.0
        on_row = y0 == row
        kind = walls[0 if drift_y < 0 else 1]
        if kind == "absorb":  # deposited at the first update, where they were
            assert np.all(want[3][on_row] == (P.AT_BOTTOM if drift_y < 0 else P.AT_TOP))
            assert np.all(want[4][on_row] == 3) and np.array_equal(want[0][on_row], x0[on_row])
        elif kind == "reflect":
            assert np.all(want[1][on_row] != row) and not want[3].any()
        else:
            assert np.all(want[1][on_row] == row)
        A = new_lattice(gpu, nx, ny, precision)
        try:
            A.set_tracers(x0, y0, stride=3)
            A.set_tracer_model(**m)
            A.step(9)
            assert_same(device_state(A), want, (walls, drift_y))
        finally:
            A.close()


@pytest.mark.parametrize("walls", [("reflect", "reflect"), ("reflect", "clamp"), ("absorb", "reflect")])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_step_larger_than_the_lattice(gpu, precision, walls):
    """D so large that amp > YDIM and amp > XDIM: reflect, then clamp; x stays where one wrap is not enough."""
    nx, ny = LATTICES[0]
    m = model(walls, diffusivity=300.0)
    assert P.amplitude(300.0, 1) > max(nx, ny)
    fields = twin_fields(gpu, nx, ny, precision, 1, [3])
    x0, y0 = seeds(nx, ny)
    x, y, laps, st, hit = fresh(x0, y0)
    folded_and_clamped = stayed = 0
    for i, (t, ux, uy) in enumerate(fields):  # the reference update by update, to see what happened
        xn, y, ln, st, hit, r = P.advect(ux, uy, x, y, laps, st, hit, 1, i, t, **ref_model(m))
        folded_and_clamped += int(np.sum(r & ((y == 0.0) | (y == ny - 1.0))))
        stayed += int(np.sum((xn == x) & (st == P.ALIVE)))
        x, laps = xn, ln
    assert folded_and_clamped > 0 and stayed > 0
    assert_in_range(x, y, nx, ny)
    A = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_tracers(x0, y0, stride=1)
        A.set_tracer_model(**m)
        A.step(3)
        assert_same(device_state(A), (x, y, laps, st, hit), walls)
    finally:
        A.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_nan_cell_leaves_its_tracers_put_and_alive(gpu, precision):
    nx, ny = LATTICES[1]
    rho, u = W.perturbed_state(nx, ny, 7)
    rho = rho.copy()
    rho[6 * nx + 5] = np.nan  # cell (5, 6)
    m = model(("absorb", "absorb"), diffusivity=0.2, drift=(0.0, -0.4))
    gx, gy = np.meshgrid(np.arange(0.25, nx, 0.5), np.arange(0.25, ny - 1, 0.5))
    x0, y0 = gx.ravel(), gy.ravel()
    A = new_lattice(gpu, nx, ny, precision, state=(rho, u))
    B = new_lattice(gpu, nx, ny, precision, state=(rho, u))
    try:
        A.set_tracers(x0, y0, stride=1)
        A.set_tracer_model(**m)
        state = fresh(x0, y0)
        for i in range(2):
            A.step(1)
            B.step(1)
            f = B.fields(["ux", "uy"])
            assert np.isnan(f["ux"][6, 5]) and np.isfinite(f["ux"][15, 25])
            before = state
            state = P.advect(f["ux"], f["uy"], *state, 1, i, B.steps, **ref_model(m))[:5]
            bad = ~np.isfinite(T.sample(f["ux"], before[0], before[1]))
            assert bad.any() and not bad.all()
            # in the reference itself: put and alive at the NaN, although the drift alone crosses the wall there
            assert np.array_equal(state[0][bad], before[0][bad]) and np.array_equal(state[1][bad], before[1][bad])
            free = ~bad & (before[3] == P.ALIVE)
            assert np.array_equal(state[3][bad], before[3][bad]) and np.all(state[0][free] != before[0][free])
            assert_same(device_state(A), state, i)
        assert np.any(state[3] == P.AT_BOTTOM)
        assert_in_range(*A.tracers()[:2], nx, ny)
    finally:
        A.close()
        B.close()


# ---- deposits -----------------------------------------------------------------------------------------

def assert_deposits_consistent(A, nx):
    x, y, laps = A.tracers()
    st, hit = A.tracer_fates()
    bottom, top = A.tracer_deposits()
    assert bottom.dtype == top.dtype == np.int64 and bottom.shape == top.shape == (nx,)
    for got, s in ((bottom, P.AT_BOTTOM), (top, P.AT_TOP)):
        assert np.array_equal(got, np.bincount(np.floor(x[st == s]).astype(np.int64), minlength=nx))
    info = A.tracer_model_info()
    assert (info["at_bottom"], info["at_top"]) == (bottom.sum(), top.sum())
    assert info["alive"] + bottom.sum() + top.sum() == x.size
    return bottom, top


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_deposits_per_column(gpu, nx, ny, precision):
    A = new_lattice(gpu, nx, ny, precision)
    try:
        x0, y0 = seeds(nx, ny)
        A.set_tracers(x0, y0, stride=3)
        A.set_tracer_model(**model(("absorb", "absorb")))
        bottom, top = assert_deposits_consistent(A, nx)
        assert not bottom.any() and not top.any()
        A.step(60)
        bottom, top = assert_deposits_consistent(A, nx)
        assert bottom.sum() >= 30 and top.sum() >= 30 and np.count_nonzero(bottom) > nx // 2
        # either output alone
        only = np.full(nx, -1, dtype=np.int64)
        A._check(A._lib.iblb_get_tracer_deposits(A.handle, None, only.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(only, top)
    finally:
        A.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_thousand_deposits_in_one_column(gpu, precision):
    """Contended atomics: every tracer released in column 7 just above an absorbing wall lands in that column."""
    nx, ny = LATTICES[0]
    n = 1000
    x0 = 7.25 + 0.5 * np.arange(n) / n
    y0 = np.full(n, 0.3)
    m = model(("absorb", "reflect"), diffusivity=0.0005, drift=(0.0, -0.5))
    fields = twin_fields(gpu, nx, ny, precision, 1, [2])
    want, _ = reference(fields, fresh(x0, y0), 1, m)
    assert np.all(want[3] == P.AT_BOTTOM) and np.all(np.floor(want[0]) == 7) and set(want[4]) == {1}
    A = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_tracers(x0, y0, stride=1)
        A.set_tracer_model(**m)
        A.step(2)
        assert_same(device_state(A), want)
        bottom, top = assert_deposits_consistent(A, nx)
        assert bottom[7] == n and bottom.sum() == n and not top.any()
        assert A.tracer_model_info()["alive"] == 0
    finally:
        A.close()


# ---- lifecycle ----------------------------------------------------------------------------------------

def test_set_state_keeps_the_model_the_fates_and_the_random_sequence(gpu):
    nx, ny, stride = *LATTICES[0], 3
    m = model(("absorb", "absorb"), diffusivity=0.3)
    x0, y0 = seeds(nx, ny)
    first = twin_fields(gpu, nx, ny, "f64", stride, [31])        # updates after 3, ..., 30; one iteration beyond
    second = twin_fields(gpu, nx, ny, "f64", stride, [30], state_seed=8)
    mid, _ = reference(first, fresh(x0, y0), stride, m)
    want, _ = reference(second, mid, stride, m, m0=len(first))
    assert np.any(mid[3] != 0) and np.sum(want[3] != 0) > np.sum(mid[3] != 0)
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        A.set_tracers(x0, y0, stride=stride)
        A.set_tracer_model(**m)
        A.step(31)
        assert_same(device_state(A), mid)
        info = A.tracer_model_info()
        A.set_state(*W.perturbed_state(nx, ny, 8))  # t = 0 again: the next update 3 iterations on, numbered 10
        assert A.tracer_model_info() == info and A.tracer_info()["updates"] == 10
        assert_same(device_state(A), mid)
        A.step(30)
        assert A.tracer_info()["updates"] == 20
        assert_same(device_state(A), want)
        late = want[3] != mid[3]
        assert np.all(want[4][late] <= 30) and np.all(want[4][late] % 3 == 0)  # hit iterations of the new state
    finally:
        A.close()


def test_set_tracers_removes_the_model(gpu):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    try:
        x0, y0 = seeds(nx, ny, 100)
        A.set_tracers(x0, y0, stride=2)
        A.set_tracer_model(**model())
        A.step(4)
        A.set_tracers(x0, y0, stride=2)  # replaced: the plain tracers again
        assert A.tracer_model_info() == {"present": False, "diffusivity": 0.0, "drift": (0.0, 0.0),
                                         "walls": ("clamp", "clamp"), "seed": 0, "alive": 0, "at_bottom": 0, "at_top": 0}
        for call in (A.tracer_fates, A.tracer_deposits):
            with pytest.raises(gpu.IblbError) as e:
                call()
            assert e.value.code == L.IBLB_ERR_STATE
        B.step(4)
        B.set_tracers(x0, y0, stride=2)
        A.step(4)
        B.step(4)
        for a, b in zip(A.tracers(), B.tracers()):
            assert np.array_equal(a, b)
        A.set_tracer_model(**model())
        A.remove_tracer_model()
        assert not A.tracer_model_info()["present"]
        A.remove_tracer_model()  # nothing to remove: still fine
        A.set_tracer_model(**model())
        A.set_tracers([], [])  # removed
        assert not A.tracer_model_info()["present"] and A.tracer_info()["n"] == 0
        with pytest.raises(gpu.IblbError) as e:
            A.set_tracer_model(**model())
        assert e.value.code == L.IBLB_ERR_STATE
    finally:
        A.close()
        B.close()


def test_checkpoints_hold_neither_the_model_nor_the_fates(gpu, tmp_path):
    nx, ny, stride = *LATTICES[1], 3
    m = model(("absorb", "absorb"), diffusivity=0.3)
    x0, y0 = seeds(nx, ny)
    fields = twin_fields(gpu, nx, ny, "f64", stride, [61])  # 20 updates; saved after 31 iterations, 10 updates
    mid, _ = reference(fields[:10], fresh(x0, y0), stride, m)
    want, _ = reference(fields, fresh(x0, y0), stride, m)
    assert np.any(mid[3] != 0) and np.sum(want[3] != 0) > np.sum(mid[3] != 0)
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        A.set_tracers(x0, y0, stride=stride)
        A.set_tracer_model(**m)
        A.step(31)
        assert_same(device_state(A), mid)
        st, hit = A.tracer_fates()
        with_model, without = str(tmp_path / "with"), str(tmp_path / "without")
        A.save_checkpoint(with_model, observers=L.OBSERVERS)
        A.remove_tracer_model()  # the twin without a model: the same state, positions, laps and schedule
        A.save_checkpoint(without, observers=L.OBSERVERS)
        assert open(with_model, "rb").read() == open(without, "rb").read()
        A.set_tracer_model(**m, status=st, iteration=hit)
        A.load_checkpoint(with_model)
        assert not A.tracer_model_info()["present"]
        assert A.tracer_info() == {"n": x0.size, "stride": stride, "updates": 10}
        A.set_tracer_model(**m, status=st, iteration=hit)  # the fates read before the save
        assert_same(device_state(A), mid)
        A.step(30)
        assert_same(device_state(A), want)  # == the uninterrupted run
    finally:
        A.close()


def test_a_pathline_repeats_a_deposited_tracers_resting_place(gpu):
    nx, ny, stride = *LATTICES[0], 3
    m = model(("absorb", "absorb"), diffusivity=0.3)
    x0, y0 = seeds(nx, ny, 200)
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        A.set_tracers(x0, y0, stride=stride)
        A.set_tracer_model(**m)
        A.set_history([], stride=stride, capacity=32, follow_tracers=True)
        A.step(60)
        h = A.history()
        x, y, laps = A.tracers()
        st, hit = A.tracer_fates()
        assert list(h["iteration"]) == list(range(3, 61, 3))
        early = (st != 0) & (hit <= 30)
        assert early.sum() >= 5 and np.any(st == 0)
        for p in np.flatnonzero(st != 0):
            after = h["iteration"] >= hit[p]
            assert after.any()
            assert np.all(h["x"][after, p] == x[p]) and np.all(h["y"][after, p] == y[p])
            assert np.all(h["laps"][after, p] == laps[p])
            assert y[p] in (0.0, ny - 1.0)
            if hit[p] > 3:
                assert not np.all(h["y"][~after, p] == y[p])
        moving = np.flatnonzero(st == 0)
        assert np.all(np.ptp(h["y"][:, moving], axis=0) > 0)
    finally:
        A.close()


# ---- errors -------------------------------------------------------------------------------------------

def test_errors_leave_the_model_and_the_fates(gpu):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        lib, h = A._lib, A.handle
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

        def mk(diffusivity=0.1, drift=(0.0, 0.0), wall=(2, 2), seed=1):
            return L.TracerModel(diffusivity, (C.c_double * 2)(*drift), (C.c_int * 2)(*wall), seed)

        def call(mod, st=None, it=None):
            return lib.iblb_set_tracer_model(h, None if mod is None else C.byref(mod), vp(st), vp(it))

        n = 6
        alive, never = np.zeros(n, np.int32), np.full(n, -1, np.int64)
        # no tracers: a state error, for a good model, for a removal and for the readers
        assert call(mk()) == L.IBLB_ERR_STATE and lib.iblb_last_error(h)
        assert call(None) == L.IBLB_ERR_STATE
        assert lib.iblb_get_tracer_fates(h, vp(alive), vp(never)) == L.IBLB_ERR_STATE
        assert lib.iblb_get_tracer_deposits(h, None, None) == L.IBLB_ERR_STATE
        assert call(mk(diffusivity=-1.0)) == L.IBLB_ERR_ARG  # the arguments are checked first
        assert not A.tracer_model_info()["present"]

        x0 = np.array([1.5, 2.5, 3.5, 4.5, 5.5, 6.5])
        y0 = np.array([0.0, ny - 1.0, 4.0, 0.0, ny - 1.0, 9.5])
        A.set_tracers(x0, y0, stride=2)
        st0 = np.array([1, 2, 0, 0, 0, 0], np.int32)
        it0 = np.array([5, 6, 77, -1, -1, -1], np.int64)
        A.set_tracer_model(0.1, (0.01, -0.02), ("absorb", "reflect"), 9, status=st0, iteration=it0)
        info = A.tracer_model_info()
        assert (info["alive"], info["at_bottom"], info["at_top"]) == (4, 1, 1)
        fates = A.tracer_fates()
        assert np.array_equal(fates[0], st0) and list(fates[1]) == [5, 6, -1, -1, -1, -1]  # alive: -1 whatever was given

        def st(i, v):
            s = st0.copy()
            s[i] = v
            return s

        bad = {
            "D < 0": (mk(diffusivity=-1e-300),), "D NaN": (mk(diffusivity=np.nan),), "D inf": (mk(diffusivity=np.inf),),
            "drift NaN": (mk(drift=(np.nan, 0.0)),), "drift inf": (mk(drift=(0.0, -np.inf)),),
            "wall 3": (mk(wall=(3, 0)),), "wall -1": (mk(wall=(0, -1)),),
            "status alone": (mk(), st0, None), "iteration alone": (mk(), None, it0),
            "status 3": (mk(), st(2, 3), it0), "status -1": (mk(), st(5, -1), it0),
            "at bottom, in the bulk": (mk(), st(2, 1), it0), "at top, in the bulk": (mk(), st(5, 2), it0),
            "at bottom, on the top row": (mk(), st(4, 1), it0), "at top, on the bottom row": (mk(), st(3, 2), it0),
        }
        for name, args in bad.items():
            assert call(*args) == L.IBLB_ERR_ARG, name
            assert lib.iblb_last_error(h), name
            assert A.tracer_model_info() == info, name
            now = A.tracer_fates()
            assert np.array_equal(now[0], fates[0]) and np.array_equal(now[1], fates[1]), name
        with pytest.raises(ValueError):
            A.set_tracer_model(walls=("absorb", "stick"))
        with pytest.raises(ValueError):
            A.set_tracer_model(status=st0[:3], iteration=it0[:3])
        # and the context still runs: the deposited ones rest, the others move
        A.step(4)
        x, y, _ = A.tracers()
        assert np.array_equal(x[:2], x0[:2]) and np.array_equal(y[:2], y0[:2]) and np.all(x[[2, 5]] != x0[[2, 5]])
    finally:
        A.close()


# ---- with IB points: invariants only ----------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", LATTICES)
def test_invariants_with_moving_ib_points(gpu, nx, ny):
    A = new_lattice(gpu, nx, ny, "f64", with_points=True)
    B = new_lattice(gpu, nx, ny, "f64", with_points=True)
    try:
        sched = moving_points(nx, ny, 60)
        A.set_lagrangian_steps(*sched)
        B.set_lagrangian_steps(*sched)
        x0, y0 = seeds(nx, ny)
        A.set_tracers(x0, y0, stride=3)
        A.set_tracer_model(**model(("absorb", "absorb")))
        B.set_tracers(x0, y0, stride=3)
        A.step(30)
        x1, y1, l1 = A.tracers()
        s1, h1 = A.tracer_fates()
        assert_deposits_consistent(A, nx)
        A.step(30)
        B.step(60)
        x2, y2, l2 = A.tracers()
        s2, h2 = A.tracer_fates()
        bottom, top = assert_deposits_consistent(A, nx)
        assert_in_range(x2, y2, nx, ny)
        done = s1 != 0
        assert done.sum() >= 30 and (s2 != 0).sum() > done.sum() and (s2 == 0).sum() >= 250
        for a, b in ((x1, x2), (y1, y2), (l1, l2), (s1, s2), (h1, h2)):  # deposited: frozen
            assert np.array_equal(a[done], b[done])
        assert np.all(y2[s2 == 1] == 0.0) and np.all(y2[s2 == 2] == ny - 1.0)
        assert np.all(h2[s2 == 0] == -1) and np.all((h2[s2 != 0] % 3 == 0) & (h2[s2 != 0] >= 3) & (h2[s2 != 0] <= 60))
        # the fluid is not disturbed (the spread's atomic order may differ in the last bits between two contexts)
        assert np.allclose(A.populations(), B.populations(), rtol=0, atol=1e-9)
    finally:
        A.close()
        B.close()
