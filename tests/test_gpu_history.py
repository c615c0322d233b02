"""The history recorder (iblb_set_history) on the GPU.  Context A carries the history; its twin B is stepped in
exactly the pieces iblb_step cuts A's calls into and, after each piece that ends on a record iteration, asked for
`sample(...)` at the probes (or `tracers()` under follow_tracers).  B's samples feed tests/history_ref.py (checked
on the CPU by tests/test_history_ref.py), and A's records, iterations and all eight statistics arrays are compared
with it through np.array_equal: a record is by definition the bits iblb_sample_points returns at that moment.

Lattices 20 x 18 and 37 x 23 (an odd size, fewer rows than a wave) of tests/test_gpu_tracers.py, f64 and f32
storage, a seeded perturbed state and a body force with both components.  The twins of the `==` comparisons carry
no IB points: the spread's atomic order may differ in the last bits between two contexts (tests/test_gpu_tracers.py).
The one case with moving IB points compares a record with iblb_sample_points on the same context with `==`, and
with the twin under that file's bound.
"""
import ctypes as C

import numpy as np
import pytest

import history_ref as H
import scalar_fields_ref as F
import scalar_ref as S
import tracer_ref as T
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_fields import BODY_FORCE
from test_gpu_scalar import seeded_c0
from test_gpu_tracers import (LATTICES, PRECISIONS, edge_seeds, fast_state, moving_points, new_lattice, point_set,
                              seeds)

pytestmark = pytest.mark.gpu

NAMES = ["rho", "ux", "uy", "vort", "sxy"]
TAU = 0.8
VALUE_BELOW = ((S.VALUE, 0.25), (S.NOFLUX, 0.0))
PATTERN = -7.0


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def code_of(gpu, call):
    with pytest.raises(gpu.IblbError) as e:
        call()
    return e.value.code


def probes(nx, ny, n):
    """n probes: the special positions of tracer_ref first, then seeded points; n = 1: the last position below
    XDIM on the top row."""
    x, y = point_set(nx, ny, max(n, 9))
    return (x[8:9], y[8:9]) if n == 1 else (x[:n], y[:n])


def assert_history_equals(A, ref, planes, what=""):
    """A's ring, iterations, record count and statistics against the restatement `ref` (planes in order)."""
    info = A.history_info()
    assert info["recorded"] == ref.recorded and info["planes"] == planes, (what, info)
    recs, its = ref.get()
    got = A.history()
    assert list(got) == ["iteration"] + planes
    assert np.array_equal(got["iteration"], its), (what, got["iteration"], its)
    for k, m in enumerate(planes):
        assert got[m].shape == recs[:, k, :].shape, (what, m)
        assert np.array_equal(got[m], recs[:, k, :], equal_nan=True), (what, m)
    st = A.history_stats()
    assert list(st) == planes
    for k, m in enumerate(planes):
        for key in H.STAT_KEYS:
            assert np.array_equal(st[m][key], ref.stats[key][k]), (what, m, key, st[m][key], ref.stats[key][k])


def snapshot(A):
    """Everything a history holds, for `unchanged` comparisons."""
    h, st = A.history(), A.history_stats()
    return A.history_info(), {k: v.copy() for k, v in h.items()}, {m: {k: v.copy() for k, v in d.items()}
                                                                  for m, d in st.items()}


def assert_same_snapshot(a, b, what=""):
    assert a[0] == b[0], what
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), (what, k)
    for m in a[2]:
        for k in a[2][m]:
            assert np.array_equal(a[2][m][k], b[2][m][k]), (what, m, k)


# ---- 1. records, iterations and statistics across calls --------------------------------------------------

@pytest.mark.parametrize("stride", [1, 5, 8])
@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_records_and_statistics_across_calls(gpu, nx, ny, precision, n, stride):
    """step(3); step(4); step(13) with the history set at t0 = 2: the records fall inside the calls and count on
    across them.  1 probe, 65 (one past a wave) and 257 (one past a workgroup)."""
    A, B = new_lattice(gpu, nx, ny, precision), new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        B.step(2)
        x, y = probes(nx, ny, n)
        A.set_history(["sxy", "ux", "rho", "vort", "uy"], x, y, stride=stride, capacity=64)
        info = A.history_info()
        assert info == {"n": n, "fields": 1 + 2 + 4 + 8 + 32, "names": NAMES, "stride": stride, "capacity": 64,
                        "flags": 0, "follow_tracers": False, "recorded": 0, "planes": NAMES}
        gx, gy = A.history_points()
        assert np.array_equal(gx, x) and np.array_equal(gy, y)
        calls = [3, 4, 13]
        plan = S.pieces(calls, 2, history=(2, stride))
        assert max(k for k, _ in plan) <= stride
        for k in calls:
            A.step(k)
        ref = H.History(len(NAMES), n, 64)
        for k, due in plan:
            B.step(k)
            if due["history"]:
                s = B.sample(NAMES, x, y)
                ref.append(np.stack([s[m] for m in NAMES]), B.steps)
        assert ref.recorded == 20 // stride
        assert_history_equals(A, ref, NAMES, f"n {n} stride {stride}")
        # the series is one: the fields moved between the records
        if ref.recorded > 1:
            assert not np.array_equal(ref.get()[0][0], ref.get()[0][-1])
        assert A.steps == B.steps == 22 and np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 2. the ring wraps -----------------------------------------------------------------------------------

@pytest.mark.parametrize("capacity", [1, 3])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_a_small_ring_keeps_the_last_records(gpu, nx, ny, precision, capacity):
    A, B = new_lattice(gpu, nx, ny, precision), new_lattice(gpu, nx, ny, precision)
    try:
        x, y = probes(nx, ny, 65)
        names = ["ux", "uy"]
        A.set_history(names, x, y, stride=2, capacity=capacity)
        A.step(7)
        A.step(9)
        ref = H.History(2, 65, capacity)
        full = H.History(2, 65, 16)
        for k in range(8):
            B.step(2)
            s = B.sample(names, x, y)
            for r in (ref, full):
                r.append(np.stack([s[m] for m in names]), B.steps)
        assert_history_equals(A, ref, names, f"capacity {capacity}")
        got = A.history()
        assert got["ux"].shape == (capacity, 65)
        assert np.array_equal(got["ux"], full.get()[0][8 - capacity:, 0, :])
        assert np.array_equal(got["iteration"], 2 * np.arange(8 - capacity + 1, 9))
        assert not np.array_equal(got["ux"], full.get()[0][:capacity, 0, :])
        # the statistics cover all 8 records, the overwritten ones included
        st = A.history_stats()
        for m in names:
            assert np.all(st[m]["count"] == 8) and np.all(st[m]["nonfinite"] == 0)
        k = names.index("ux")
        assert np.array_equal(st["ux"]["max"], full.get()[0][:, k, :].max(axis=0))
        assert np.any(st["ux"]["max_rec"] < 8 - capacity) or np.any(st["ux"]["min_rec"] < 8 - capacity)
        # a stretch outside the window: IBLB_ERR_ARG, nothing written
        lib, h = A._lib, A.handle
        out = np.full(capacity * 2 * 65 + 8, PATTERN)
        it = np.full(capacity + 8, -7, dtype=np.int64)
        oldest = 8 - capacity
        for first, count in [(oldest - 1, 1), (oldest, capacity + 1), (8, 1), (oldest, -1), (-1, 1), (9, 0)]:
            assert lib.iblb_get_history(h, first, count, p(out), p(it)) == L.IBLB_ERR_ARG, (first, count)
            assert np.all(out == PATTERN) and np.all(it == -7), (first, count)
        assert lib.iblb_get_history(h, oldest, 1, None, None) == L.IBLB_ERR_ARG
        # inside it: either output alone, and reading does not drain
        assert lib.iblb_get_history(h, 8, 0, p(out), p(it)) == L.IBLB_OK and np.all(out == PATTERN)
        assert lib.iblb_get_history(h, 7, 1, None, p(it)) == L.IBLB_OK and it[0] == 16 and it[1] == -7
        assert lib.iblb_get_history(h, 7, 1, p(out), None) == L.IBLB_OK
        assert np.array_equal(out[:130], full.get()[0][7].ravel()) and np.all(out[130:] == PATTERN)
        assert np.array_equal(A.history(oldest, capacity)["uy"], got["uy"])
    finally:
        A.close()
        B.close()


# ---- 3. with a scalar ------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [4, 6])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_records_sample_the_scalar_after_its_event(gpu, nx, ny, precision, stride):
    """The scalar every 4 iterations, records every `stride` (4: every record shares its iteration with an event;
    6: the record after iteration 12 does), over step(9); step(11).  The series built from C before the event
    differs."""
    A, B = new_lattice(gpu, nx, ny, precision), new_lattice(gpu, nx, ny, precision)
    try:
        c0 = seeded_c0(nx, ny)
        for lat in (A, B):
            lat.set_scalar(c0, tau=TAU, stride=4, walls=VALUE_BELOW)
        x, y = probes(nx, ny, 65)
        names = ["c", "cux", "cuy"]
        A.set_history(names, x, y, stride=stride, capacity=8)
        calls = [9, 11]
        plan = S.pieces(calls, 0, scalar=(0, 4), history=(0, stride))
        shared = [d["scalar"] for _, d in plan if d["history"]]
        assert shared == ([True] * 5 if stride == 4 else [False, True, False])
        for k in calls:
            A.step(k)
        ref, wrong = H.History(3, 65, 8), H.History(3, 65, 8)
        for k, due in plan:
            g_prev = B.scalar_populations()
            B.step(k)
            if due["history"]:
                s = B.sample(names, x, y)
                ref.append(np.stack([s[m] for m in names]), B.steps)
                f = B.fields(["ux", "uy"])
                now = F.scalar_fields(B.scalar_populations(), f["ux"], f["uy"])
                assert np.array_equal(H.record_of(now, names, x, y), ref.get()[0][-1])  # the restatement is B's sample
                wrong.append(H.record_of(F.scalar_fields(g_prev, f["ux"], f["uy"]), names, x, y), B.steps)
        assert_history_equals(A, ref, names, f"stride {stride}")
        assert not np.array_equal(wrong.get()[0], ref.get()[0]), "the order of the event and the record is untested"
        assert np.array_equal(A.scalar_populations(), B.scalar_populations())
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 4. pathlines ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("names", [["ux", "uy"], []])
@pytest.mark.parametrize("stride", [1, 5])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_pathlines_follow_the_tracers(gpu, nx, ny, precision, stride, names):
    state = fast_state(nx, ny)
    A, B = (new_lattice(gpu, nx, ny, precision, state=state) for _ in range(2))
    try:
        x0, y0 = edge_seeds(nx, ny)
        n = x0.size
        for lat in (A, B):
            lat.set_tracers(x0, y0, stride=stride)
        A.set_history(names, stride=stride, capacity=32, follow_tracers=True)
        planes = ["x", "y", "laps"] + names
        info = A.history_info()
        assert info["n"] == n and info["follow_tracers"] and info["flags"] == L.HIST_TRACERS
        assert info["fields"] == sum(L.READ_FIELDS[m] for m in names) and info["planes"] == planes
        assert code_of(gpu, A.history_points) == L.IBLB_ERR_STATE
        calls = [4] if stride == 1 else [3, 4, 8]
        plan = S.pieces(calls, 0, tracers=(0, stride), history=(0, stride))
        for k in calls:
            A.step(k)
        ref = H.History(len(planes), n, 32)
        for k, due in plan:
            B.step(k)
            if due["history"]:
                assert due["tracers"]
                tx, ty, tl = B.tracers()
                rows = [tx, ty, tl.astype(np.float64)]
                if names:
                    s = B.sample(names, tx, ty)
                    rows += [s[m] for m in names]
                ref.append(np.stack(rows), B.steps)
        assert ref.recorded == sum(calls) // stride
        assert_history_equals(A, ref, planes, f"stride {stride} {names}")
        # the case is not empty: a wrap each way within the records at both strides, and at stride 1 (the first
        # update sees the seeded velocity; by iteration 5 the walls have slowed the rows next to them) a clamp at
        # each wall
        got = A.history()
        assert np.any(got["laps"] > 0) and np.any(got["laps"] < 0)
        if stride == 1:
            assert np.any((got["y"] == 0.0) & (y0 > 0.0)) and np.any((got["y"] == ny - 1.0) & (y0 < ny - 1.0))
        # a record holds the positions after that iteration's update
        tx, ty, tl = A.tracers()
        assert np.array_equal(got["x"][-1], tx) and np.array_equal(got["y"][-1], ty) and np.array_equal(got["laps"][-1], tl)
        # the tracers can be neither replaced nor removed meanwhile, and nothing changes
        before = snapshot(A)
        assert code_of(gpu, lambda: A.set_tracers(x0[:3], y0[:3], stride=1)) == L.IBLB_ERR_STATE
        assert code_of(gpu, lambda: A.set_tracers([], [])) == L.IBLB_ERR_STATE
        assert A.tracer_info() == B.tracer_info()
        for a, b in zip(A.tracers(), (tx, ty, tl)):
            assert np.array_equal(a, b)
        assert_same_snapshot(snapshot(A), before)
        A.remove_history()
        A.set_tracers([], [])
        assert A.tracer_info()["n"] == 0
        assert code_of(gpu, lambda: A.set_history(names, follow_tracers=True)) == L.IBLB_ERR_STATE  # no tracers
        assert A.history_info()["n"] == 0
    finally:
        A.close()
        B.close()


# ---- 5. a record meets an owed IB force ---------------------------------------------------------------------

def test_a_record_under_moving_ib_points(gpu):
    """Moving IB points (a schedule), records every 3 iterations over step(3); step(9).  The record that ends a call
    equals iblb_sample_points on A itself with `==`: the same context, the same state and force.  Against the twin B
    the spread's atomic order may differ in the last bits, so there the bound is 1e-9 * (|v| + 1), the project's f64
    parity bound for u (tests/test_gpu_bulk.py, tests/test_gpu_tracers.py)."""
    nx, ny = LATTICES[1]
    A, B, Cn = (new_lattice(gpu, nx, ny, "f64", with_points=k < 2) for k in range(3))
    try:
        sched = moving_points(nx, ny, 12)
        A.set_lagrangian_steps(*sched)
        B.set_lagrangian_steps(*sched)
        x, y = probes(nx, ny, 65)
        names = ["ux", "uy"]
        for lat in (A, Cn):
            lat.set_history(names, x, y, stride=3, capacity=8)
        A.step(3)
        own = A.sample(names, x, y)
        got = A.history()
        assert got["iteration"].tolist() == [3]
        for m in names:
            assert np.array_equal(got[m][0], own[m]), m
        A.step(9)
        own = A.sample(names, x, y)
        got = A.history()
        assert got["iteration"].tolist() == [3, 6, 9, 12]
        for m in names:
            assert np.array_equal(got[m][-1], own[m]), m
        for r in range(4):
            B.step(3)
            s = B.sample(names, x, y)
            for m in names:
                err = np.abs(got[m][r] - s[m])
                print(f"record {r} {m}: max |d| {err.max():.3e}")
                assert np.all(err <= 1e-9 * (np.abs(s[m]) + 1.0)), (r, m, err.max())
        # the IB force reached the records: the same run without points records other values
        Cn.step(12)
        assert not np.array_equal(Cn.history()["ux"], got["ux"])
    finally:
        for lat in (A, B, Cn):
            lat.close()


# ---- 6. the history changes nothing else --------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_the_history_changes_nothing_else(gpu, nx, ny, precision):
    """Stride 8 >= K: D, without a history, is stepped in the pieces A's calls are cut into.  The populations agree
    after every call, the deep launches and their iterations are D's, and after remove_history A is D."""
    A, D = new_lattice(gpu, nx, ny, precision), new_lattice(gpu, nx, ny, precision)
    try:
        x, y = probes(nx, ny, 65)
        A.set_history(NAMES, x, y, stride=8, capacity=4)
        calls = [9, 11, 20]
        t = 0
        for k in calls:
            A.step(k)
            for q, _ in S.pieces([k], t, history=(0, 8)):
                D.step(q)
            t += k
            assert np.array_equal(A.populations(), D.populations()), t
        assert A.history_info()["recorded"] == 5
        ta, td = A.timing(), D.timing()
        for k in ("deep_launches", "deep_iterations"):
            assert ta[k] == td[k], (k, ta[k], td[k])
        assert td["deep_launches"] > 0  # the path compared is the deep sweep
        A.remove_history()
        assert A.history_info() == {"n": 0, "fields": 0, "names": [], "stride": 0, "capacity": 0, "flags": 0,
                                    "follow_tracers": False, "recorded": 0, "planes": []}
        for call in (A.history, A.history_stats, A.history_points, A.reset_history):
            assert code_of(gpu, call) == L.IBLB_ERR_STATE
        A.step(14)
        D.step(14)
        ta1, td1 = A.timing(), D.timing()
        for k in ("deep_launches", "deep_iterations"):
            assert ta1[k] - ta[k] == td1[k] - td[k], k
        assert td1["deep_launches"] - td["deep_launches"] > 0
        assert np.array_equal(A.populations(), D.populations())
    finally:
        A.close()
        D.close()


# ---- 7. life cycle ------------------------------------------------------------------------------------------

def test_set_state_keeps_reset_zeroes_and_a_checkpoint_drops_the_history(gpu, tmp_path):
    nx, ny = LATTICES[0]
    A, B = new_lattice(gpu, nx, ny, "f64"), new_lattice(gpu, nx, ny, "f64")
    try:
        x, y = probes(nx, ny, 65)
        names = ["ux", "uy"]
        ref = H.History(2, 65, 16)

        def follow(plan):
            for k, due in plan:
                B.step(k)
                if due:
                    s = B.sample(names, x, y)
                    ref.append(np.stack([s[m] for m in names]), B.steps)

        A.set_history(names, x, y, stride=3, capacity=16)
        A.step(4)  # one record, one iteration into the next interval
        follow([(3, True), (1, False)])
        assert_history_equals(A, ref, names, "before set_state")
        # a new state: records, statistics and the count stay, the next record is `stride` iterations on
        rho, u = W.perturbed_state(nx, ny, 8)
        A.set_state(rho, u)
        B.set_state(rho, u)
        assert_history_equals(A, ref, names, "after set_state")
        A.step(2)
        assert A.history_info()["recorded"] == 1
        A.step(4)
        follow([(2, False), (1, True), (3, True)])
        assert ref.get()[1].tolist() == [3, 3, 6]  # iterations count from the new state
        assert_history_equals(A, ref, names, "re-based")
        # reset: nothing recorded, nothing seen, the probes kept, t0 = now
        A.reset_history()
        ref.reset()
        assert_history_equals(A, ref, names, "after reset")
        st = A.history_stats()["ux"]
        assert np.all(st["min"] == np.inf) and np.all(st["max"] == -np.inf) and np.all(st["min_rec"] == -1)
        assert np.all(st["max_rec"] == -1) and not st["count"].any() and not st["sum"].any()
        gx, gy = A.history_points()
        assert np.array_equal(gx, x) and np.array_equal(gy, y)
        A.step(3)
        follow([(3, True)])
        assert_history_equals(A, ref, names, "after reset and a record")
        # a checkpoint holds no history, and loading one removes it
        ck = str(tmp_path / "ck")
        A.save_checkpoint(ck, observers=L.OBSERVERS)
        assert A.history_info()["recorded"] == 1
        A.load_checkpoint(ck)
        assert A.history_info()["n"] == 0
        A.step(5)
        B.step(5)
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


def test_the_scalar_stays_while_the_history_records_it(gpu):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        x, y = probes(nx, ny, 5)
        assert code_of(gpu, lambda: A.set_history(["c"], x, y)) == L.IBLB_ERR_STATE  # no scalar yet
        assert A.history_info()["n"] == 0
        c0 = seeded_c0(nx, ny)
        A.set_scalar(c0, tau=TAU, stride=2)
        A.set_history(["ux", "c"], x, y, stride=2, capacity=4)
        A.step(2)
        before = snapshot(A)
        assert code_of(gpu, A.remove_scalar) == L.IBLB_ERR_STATE
        assert A.scalar_info()["stride"] == 2
        assert_same_snapshot(snapshot(A), before)
        A.set_scalar(c0 + 1.0, tau=0.9, stride=2)  # replacing is allowed: the history goes on with the new one
        A.step(2)
        h = A.history()
        assert h["iteration"].tolist() == [2, 4]
        assert np.array_equal(h["c"][1], A.sample("c", x, y)["c"]) and np.all(h["c"][1] > h["c"][0] + 0.5)
        A.set_history(["ux"], x, y, stride=2, capacity=4)  # no scalar bit any more
        A.remove_scalar()
        A.step(2)
        assert A.history_info()["recorded"] == 1
    finally:
        A.close()


def test_argument_errors_leave_the_previous_history(gpu):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    try:
        x, y = probes(nx, ny, 65)
        A.set_history(["ux", "uy"], x, y, stride=2, capacity=3)
        A.step(9)
        before = snapshot(A)
        assert before[0]["recorded"] == 4
        lib, h = A._lib, A.handle
        good = np.array([1.5, 2.5, 3.5])
        bad = {
            "n < 0": (-1, good, good, 2, 1, 4, 0),
            "x NULL": (3, None, good, 2, 1, 4, 0),
            "y NULL": (3, good, None, 2, 1, 4, 0),
            "fields 0": (3, good, good, 0, 1, 4, 0),
            "unknown field": (3, good, good, 128, 1, 4, 0),
            "unknown field, following": (0, None, None, 2048, 1, 4, L.HIST_TRACERS),
            "stride 0": (3, good, good, 2, 0, 4, 0),
            "capacity 0": (3, good, good, 2, 1, 0, 0),
            "capacity < 0": (3, good, good, 2, 1, -5, 0),
            "unknown flag": (3, good, good, 2, 1, 4, 2),
            "x = XDIM": (3, np.array([1.5, float(nx), 3.5]), good, 2, 1, 4, 0),
            "x < 0": (3, np.array([1.5, -1e-9, 3.5]), good, 2, 1, 4, 0),
            "y > YDIM-1": (3, good, np.array([1.5, np.nextafter(ny - 1.0, ny), 2.0]), 2, 1, 4, 0),
            "NaN x": (3, np.array([np.nan, 2.5, 3.5]), good, 2, 1, 4, 0),
            "inf y": (3, good, np.array([1.5, np.inf, 2.0]), 2, 1, 4, 0),
        }
        for name, (n, bx, by, fields, stride, cap, flags) in bad.items():
            assert lib.iblb_set_history(h, n, p(bx), p(by), fields, stride, cap, flags) == L.IBLB_ERR_ARG, name
            assert lib.iblb_last_error(h), name
            assert_same_snapshot(snapshot(A), before, name)
        # state errors and an allocation that cannot succeed leave it too
        assert lib.iblb_set_history(h, 3, p(good), p(good), 4096, 1, 4, 0) == L.IBLB_ERR_STATE  # no scalar
        assert lib.iblb_set_history(h, 0, None, None, 0, 1, 4, L.HIST_TRACERS) == L.IBLB_ERR_STATE  # no tracers
        assert lib.iblb_set_history(h, 3, p(good), p(good), 2, 1, 1 << 60, 0) == L.IBLB_ERR_NOMEM
        assert_same_snapshot(snapshot(A), before, "state / memory errors")
        assert lib.iblb_get_history_stats(h, None, None, None, None, None, None, None, None) == L.IBLB_ERR_ARG
        with pytest.raises(ValueError):
            A.set_history(["pressure"], x, y)
        # and it still records
        A.step(1)
        assert A.history_info()["recorded"] == 5 and A.history()["iteration"].tolist() == [6, 8, 10]
        # a replacement starts at zero
        A.set_history(["rho"], good, good, stride=1, capacity=2)
        info = A.history_info()
        assert (info["n"], info["recorded"], info["names"], info["capacity"]) == (3, 0, ["rho"], 2)
        assert A.history()["rho"].shape == (0, 3) and not A.history_stats()["rho"]["count"].any()
    finally:
        A.close()


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
            for call in (lambda: s.set_history("ux", x, y), lambda: s.set_history("ux", follow_tracers=True)):
                assert code_of(gpu, call) == L.IBLB_ERR_UNSUPPORTED
                msg = s._lib.iblb_last_error(s.handle)
                assert msg and len(msg.decode()) > 0
            assert s.history_info()["n"] == 0
            s.remove_history()  # removing nothing is allowed anywhere
    finally:
        for s in slabs:
            s.close()
