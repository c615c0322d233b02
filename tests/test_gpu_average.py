"""The averaged fields of iblb_set_average on the GPU against tests/average_ref.py (checked on the CPU by
tests/test_average_ref.py) applied to what Lattice.fields returns for a twin lattice stepped in the pieces
iblb_step cuts its calls into.

Lattices 20 x 18, 37 x 23 (an odd size, fewer rows than a wave) and 16 x 300 (more rows than a 256-lane
workgroup, not a multiple of 64), f64 and f32 storage, a seeded perturbed state and a body force with both
components.

The sums are compared with `==` (np.array_equal): the device evaluates a sample with the functions
iblb_get_fields uses and adds it with one rounding per operation in sample order, which is what the numpy
twin does.  The lattices of the `==` comparisons carry no IB points: the spread's atomic order may differ in
the last bits between two contexts (tests/test_gpu_tracers.py).  With moving IB points the bound is
1e-9 * samples * (1 + max |v|): the project's f64 parity bound for fields (tests/test_gpu_bulk.py), once per
sample added.
"""
import ctypes as C

import numpy as np
import pytest

import average_ref as R
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_fields import BODY_FORCE
from test_gpu_tracers import host_trajectory, moving_points, new_lattice, seeds

pytestmark = pytest.mark.gpu

LATTICES = [(20, 18), (37, 23), (16, 300)]
PRECISIONS = ["f64", "f32"]
ALL = ["rho", "ux", "uy", "vort", "sxx", "sxy", "syy"]


def twin_samples(B, plan, names=ALL, window=None):
    """Step the twin B in the pieces of `plan` and read the fields at every average sample."""
    out = []
    for n, _, sample in plan:
        B.step(n)
        if sample:
            out.append({k: v.copy() for k, v in B.fields(names, window).items()})
    return out


def assert_bins_equal(A, ref, what):
    """Every plane and count of every bin of lattice A equals the reference bins, bit for bit."""
    for b, r in enumerate(ref):
        got = A.average(b)
        assert got["samples"] == r["samples"], (what, b)
        assert list(got["sum"]) == list(r["sum"]), (what, b)
        for n in r["sum"]:
            assert got["sum"][n].shape == r["sum"][n].shape, (what, b, n)
            assert np.array_equal(got["sum"][n], r["sum"][n]), (what, b, n, np.max(np.abs(got["sum"][n] - r["sum"][n])))
        assert (got["sum_sq"] is None) == (r["sum_sq"] is None), (what, b)
        if r["sum_sq"] is not None:
            for n in r["sum_sq"]:
                assert np.array_equal(got["sum_sq"][n], r["sum_sq"][n]), (what, b, n)
        assert (got["sum_uxuy"] is None) == (r["sum_uxuy"] is None), (what, b)
        if r["sum_uxuy"] is not None:
            assert np.array_equal(got["sum_uxuy"], r["sum_uxuy"]), (what, b)


# ---- 1. the sums equal the twin --------------------------------------------------------------------------

@pytest.mark.parametrize("nbins", [1, 3])
@pytest.mark.parametrize("stride", [1, 5, 7, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_sums_equal_the_twin(gpu, nx, ny, precision, stride, nbins):
    """step(3); step(4); step(13) with all seven fields and both flags set at t0 = 2: the samples fall inside
    the calls and count on across them.  Where those 20 iterations give no bin a second sample (stride 7 and 8
    with three bins: two samples) one more call of stride * nbins iterations follows and everything is compared
    again, so that every case adds onto a sum that is not zero."""
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        B.step(2)
        A.set_average(ALL, stride=stride, nbins=nbins, squares=True, uxuy=True)
        info = A.average_info()
        assert info["window"] == (0, 0, nx, ny, 1, 1) and info["names"] == ALL and info["fields"] == 127
        assert (info["stride"], info["nbins"], info["flags"], info["samples_total"]) == (stride, nbins, 3, 0)
        calls = [3, 4, 13]
        plan = R.pieces(calls, 2, average=(2, stride))
        assert sum(p[0] for p in plan) == 20 and max(p[0] for p in plan) <= max(stride, 1)
        for n in calls:
            A.step(n)
        samples = twin_samples(B, plan)
        assert len(samples) == 20 // stride
        ref = R.accumulate(samples, nbins, squares=True, uxuy=True)
        assert_bins_equal(A, ref, "first 20 iterations")
        assert A.average_info()["samples_total"] == len(samples)
        if max(r["samples"] for r in ref) < 2:
            more = stride * nbins
            A.step(more)
            samples += twin_samples(B, R.pieces([more], 22, average=(2, stride)))
            ref = R.accumulate(samples, nbins, squares=True, uxuy=True)
            assert_bins_equal(A, ref, "after one more call")
        assert A.steps == B.steps
        assert np.array_equal(A.populations(), B.populations())
        # the case is not empty: a bin with at least two samples, and there u_x fluctuates somewhere
        full = [r for r in ref if r["samples"] >= 2]
        assert full
        got = A.average(ref.index(full[0]))
        n = float(got["samples"])
        mean = got["sum"]["ux"] / n
        assert np.any(got["sum_sq"]["ux"] / n - mean * mean > 0)
        assert np.array_equal(A.mean(ref.index(full[0]))["ux"], mean)
    finally:
        A.close()
        B.close()


# ---- 2. windows ------------------------------------------------------------------------------------------

def windows(nx, ny):
    """(3, 1, ., ., 3, 2) holds as many samples as fit: its last sample is the last column on 37 x 23 and
    16 x 300 and the last row on 20 x 18 and 16 x 300."""
    w = {
        "whole": None,
        "offset(3,1) stride(3,2)": (3, 1, (nx - 4) // 3 + 1, (ny - 2) // 2 + 1, 3, 2),
        "corner X,Y": (nx - 1, ny - 1, 1, 1, 1, 1),
    }
    if (nx, ny) == (16, 300):
        w["one column, every row"] = (5, 0, 1, ny, 1, 1)
    return w


def test_the_strided_window_reaches_the_last_column_and_row():
    x_end = {(nx, ny): 3 + 3 * (windows(nx, ny)["offset(3,1) stride(3,2)"][2] - 1) for nx, ny in LATTICES}
    y_end = {(nx, ny): 1 + 2 * (windows(nx, ny)["offset(3,1) stride(3,2)"][3] - 1) for nx, ny in LATTICES}
    assert x_end[(16, 300)] == 15 and y_end[(16, 300)] == 299 and x_end[(37, 23)] == 36 and y_end[(20, 18)] == 17


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_windows(gpu, nx, ny, precision):
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.step(2)
        B.step(2)
        for name, w in windows(nx, ny).items():
            t = A.steps
            A.set_average(ALL, window=w, stride=5, nbins=2, squares=True, uxuy=True)  # replaces the previous set
            A.step(17)
            plan = R.pieces([17], t, average=(t, 5))
            samples = twin_samples(B, plan, window=w)
            assert len(samples) == 3
            ref = R.accumulate(samples, 2, squares=True, uxuy=True)
            assert [r["samples"] for r in ref] == [2, 1]
            shape = (ny, nx) if w is None else (w[3], w[2])
            assert A.average(0)["sum"]["rho"].shape == shape and A.average(0)["sum_uxuy"].shape == shape, name
            assert A.average_info()["window"] == ((0, 0, nx, ny, 1, 1) if w is None else w), name
            assert_bins_equal(A, ref, name)
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 3. a subset given out of order -----------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_subset_out_of_order_and_planes_not_requested(gpu, precision):
    nx, ny = LATTICES[1]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_average(["uy", "rho"], stride=2)
        A.step(5)
        samples = twin_samples(B, R.pieces([5], 0, average=(0, 2)), names=["rho", "uy"])
        got = A.average()
        assert list(got["sum"]) == ["rho", "uy"] and got["sum_sq"] is None and got["sum_uxuy"] is None
        assert A.average_info()["names"] == ["rho", "uy"] and A.average_info()["flags"] == 0
        assert_bins_equal(A, R.accumulate(samples, 1), "rho | uy")
        # at the C level a plane that was not requested is refused, nothing written
        lib, h = A._lib, A.handle
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        s, q = np.full(2 * ny * nx, -7.0), np.full(2 * ny * nx, -7.0)
        n = C.c_longlong(-3)
        assert lib.iblb_get_average(h, 0, p(s), p(q), None, C.byref(n)) == L.IBLB_ERR_ARG
        assert lib.iblb_get_average(h, 0, p(s), None, p(q), C.byref(n)) == L.IBLB_ERR_ARG
        assert np.all(s == -7.0) and np.all(q == -7.0) and n.value == -3
        assert lib.iblb_get_average(h, 0, None, None, None, C.byref(n)) == L.IBLB_OK and n.value == 2
        with pytest.raises(ValueError):
            A.set_average(["pressure"])
    finally:
        A.close()
        B.close()


# ---- 4. the boot phase ------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_set_before_the_first_step(gpu, nx, ny, precision):
    A = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_average(ALL, stride=1, squares=True, uxuy=True)
        got = A.average()
        assert got["samples"] == 0 and A.average_info()["samples_total"] == 0  # no sample at t0
        assert not any(v.any() for v in got["sum"].values()) and not got["sum_uxuy"].any()
        A.step(1)
        got, f = A.average(), A.fields(ALL)
        assert got["samples"] == 1
        for n in ALL:
            assert np.array_equal(got["sum"][n], f[n]), n
            assert np.array_equal(got["sum_sq"][n], f[n] * f[n]), n
        assert np.array_equal(got["sum_uxuy"], f["ux"] * f["uy"])
        assert np.max(np.abs(got["sum"]["sxy"])) > 0 and np.max(np.abs(got["sum"]["vort"])) > 0
    finally:
        A.close()


# ---- 5. with tracers --------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES[:2])
def test_with_tracers(gpu, nx, ny, precision):
    """Tracers every 3 and samples every 5 iterations over step(17): the call is cut at the union of both."""
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    Bt = new_lattice(gpu, nx, ny, precision)
    try:
        x0, y0 = seeds(nx, ny)
        A.set_tracers(x0, y0, stride=3)
        A.set_average(ALL, stride=5, nbins=2, squares=True, uxuy=True)
        A.step(17)
        plan = R.pieces([17], 0, tracers=(0, 3), average=(0, 5))
        x, y, laps, path = host_trajectory(Bt, x0, y0, np.zeros(x0.size, dtype=np.int32), 3, [(n, ut) for n, ut, _ in plan])
        gx, gy, gl = A.tracers()
        assert np.median(path) > 0
        assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gl, laps)
        assert_bins_equal(A, R.accumulate(twin_samples(B, plan), 2, squares=True, uxuy=True), "with tracers")
        assert A.tracer_info()["updates"] == 5 and A.average_info()["samples_total"] == 3
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()
        Bt.close()


# ---- 6. with moving IB points -----------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", LATTICES)
def test_with_moving_ib_points(gpu, nx, ny):
    A = new_lattice(gpu, nx, ny, "f64", with_points=True)
    B = new_lattice(gpu, nx, ny, "f64", with_points=True)
    Cn = new_lattice(gpu, nx, ny, "f64")
    try:
        sched = moving_points(nx, ny, 12)
        A.set_lagrangian_steps(*sched)
        B.set_lagrangian_steps(*sched)
        for lat in (A, Cn):
            lat.set_average(ALL, stride=3, nbins=2)
            lat.step(12)
        samples = twin_samples(B, R.pieces([12], 0, average=(0, 3)))
        ref = R.accumulate(samples, 2)
        assert [r["samples"] for r in ref] == [2, 2]
        for b, r in enumerate(ref):
            got, free = A.average(b), Cn.average(b)
            assert got["samples"] == r["samples"] == free["samples"]
            for n in ALL:
                vmax = max(np.max(np.abs(s[n])) for s in samples[b::2])
                bound = 1e-9 * r["samples"] * (1.0 + vmax)
                err = np.max(np.abs(got["sum"][n] - r["sum"][n]))
                print(f"{nx}x{ny} bin {b} {n}: max |d sum| {err:.3e} bound {bound:.3e}")
                assert err <= bound, (b, n, err, bound)
            # the IB force reached the sums: the same run without points gives others
            assert not np.array_equal(got["sum"]["ux"], free["sum"]["ux"]), b
            assert not np.array_equal(got["sum"]["uy"], free["sum"]["uy"]), b
    finally:
        A.close()
        B.close()
        Cn.close()


# ---- 7. removal restores the old path; a stride of K keeps the deep sweep --------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_removing_the_average_restores_the_old_path(gpu, precision):
    nx, ny = LATTICES[1]
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        A.set_average(ALL, stride=1, squares=True, uxuy=True)
        A.step(3)
        for _ in range(3):  # the pieces A's call was cut into
            B.step(1)
        A.set_average([])
        assert A.average_info()["fields"] == 0 and A.average_info()["samples_total"] == 0
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
        A.set_average(["rho", "ux", "uy"], stride=7)
        ta, tb = A.timing(), B.timing()
        A.step(14)
        for n, _, _ in R.pieces([14], 7, average=(7, 7)):
            assert n == 7
            B.step(n)
        ta1, tb1 = A.timing(), B.timing()
        for k in ("deep_launches", "deep_iterations"):
            assert ta1[k] - ta[k] == tb1[k] - tb[k], (k, ta[k], ta1[k], tb[k], tb1[k])
        assert tb1["deep_launches"] - tb["deep_launches"] > 0
        assert A.average()["samples"] == 2
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 8. lifecycle ------------------------------------------------------------------------------------------

def test_reset_set_state_and_checkpoint(gpu, tmp_path):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    names = ["rho", "ux", "uy"]
    try:
        A.set_average(names, stride=2, nbins=2, squares=True, uxuy=True)
        A.step(5)  # samples after iterations 2 and 4
        B.step(5)
        assert [A.average(b)["samples"] for b in (0, 1)] == [1, 1] and A.average(0)["sum"]["rho"].any()
        # reset: sums and counts zero, t0 = 5, the next sample is number 0 after iteration 7
        A.reset_average()
        for b in (0, 1):
            got = A.average(b)
            assert got["samples"] == 0 and not got["sum_uxuy"].any()
            assert not any(v.any() for v in got["sum"].values()) and not any(v.any() for v in got["sum_sq"].values())
        assert A.average_info()["samples_total"] == 0
        A.step(1)
        assert A.average_info()["samples_total"] == 0
        A.step(1)
        samples = twin_samples(B, [(2, False, True)], names)
        assert_bins_equal(A, R.accumulate(samples, 2, squares=True, uxuy=True), "after the reset")
        # a new state: sums and counts stay, the next sample comes `stride` iterations on
        kept = A.average(0)
        rho, u = W.perturbed_state(nx, ny, 8)
        A.set_state(rho, u)
        B.set_state(rho, u)
        assert A.average_info()["samples_total"] == 1 and A.average(0)["samples"] == 1
        assert np.array_equal(A.average(0)["sum"]["ux"], kept["sum"]["ux"])
        A.step(1)
        assert A.average_info()["samples_total"] == 1
        A.step(1)
        samples += twin_samples(B, [(1, False, False), (1, False, True)], names)
        assert A.average_info()["samples_total"] == 2
        assert_bins_equal(A, R.accumulate(samples, 2, squares=True, uxuy=True), "after set_state")
        # a checkpoint holds no averages
        ck = str(tmp_path / "ck")
        A.save_checkpoint(ck)
        A.load_checkpoint(ck)
        assert A.average_info()["fields"] == 0
        lib, h = A._lib, A.handle
        buf = np.full(3 * ny * nx, -7.0)
        n = C.c_longlong(-3)
        assert lib.iblb_reset_average(h) == L.IBLB_ERR_STATE
        assert lib.iblb_get_average(h, 0, buf.ctypes.data_as(C.c_void_p), None, None, C.byref(n)) == L.IBLB_ERR_STATE
        assert np.all(buf == -7.0) and n.value == -3 and lib.iblb_last_error(h)
        with pytest.raises(gpu.IblbError):
            A.average()
        A.step(5)
        B.step(5)
        assert np.array_equal(A.populations(), B.populations())
    finally:
        A.close()
        B.close()


# ---- 9. errors leave everything as it was --------------------------------------------------------------

def test_argument_errors_leave_the_average_as_it_was(gpu):
    nx, ny = LATTICES[0]
    A = new_lattice(gpu, nx, ny, "f64")
    B = new_lattice(gpu, nx, ny, "f64")
    names = ["rho", "ux", "uy"]
    try:
        A.set_average(names, window=(1, 2, 5, 4, 2, 3), stride=2, nbins=2, squares=True, uxuy=True)
        A.step(2)
        samples = twin_samples(B, [(2, False, True)], names, (1, 2, 5, 4, 2, 3))
        info = A.average_info()
        lib, h = A._lib, A.handle
        RHO, UX, UY = 1, 2, 4
        good = L.Window(0, 0, 4, 4, 1, 1)
        bad_sets = {
            "unknown bit 128": (good, RHO | 128, 1, 1, 0),
            "flag 4": (good, RHO, 1, 1, 4),
            "UXUY without UY": (good, RHO | UX, 1, 1, L.AVG_UXUY),
            "UXUY without UX": (good, RHO | UY, 1, 1, L.AVG_UXUY),
            "stride 0": (good, RHO, 0, 1, 0),
            "nbins 0": (good, RHO, 1, 0, 0),
            "no field with a window": (good, 0, 1, 1, 0),
            "a window past the last column": (L.Window(nx - 2, 0, 2, 2, 2, 1), RHO, 1, 1, 0),
            "a window past the last row": (L.Window(0, 0, 2, ny + 1, 1, 1), RHO, 1, 1, 0),
            "a window of no samples": (L.Window(0, 0, 0, 2, 1, 1), RHO, 1, 1, 0),
        }
        for name, (w, fields, stride, nbins, flags) in bad_sets.items():
            assert lib.iblb_set_average(h, C.byref(w), fields, stride, nbins, flags) == L.IBLB_ERR_ARG, name
            assert lib.iblb_last_error(h), name
            assert A.average_info() == info, name
        assert lib.iblb_set_average(h, None, RHO, 0, 1, 0) == L.IBLB_ERR_ARG
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        s, q, xy = np.full(3 * 20, -7.0), np.full(3 * 20, -7.0), np.full(20, -7.0)
        n = C.c_longlong(-3)
        for bin in (2, -1):
            assert lib.iblb_get_average(h, bin, p(s), p(q), p(xy), C.byref(n)) == L.IBLB_ERR_ARG, bin
        assert np.all(s == -7.0) and np.all(q == -7.0) and np.all(xy == -7.0) and n.value == -3
        # the set is as it was, its sums too, and the next sample still matches the twin
        assert A.average_info() == info
        assert_bins_equal(A, R.accumulate(samples, 2, squares=True, uxuy=True), "after the refused calls")
        A.step(2)
        samples += twin_samples(B, [(2, False, True)], names, (1, 2, 5, 4, 2, 3))
        assert_bins_equal(A, R.accumulate(samples, 2, squares=True, uxuy=True), "the next sample")
    finally:
        A.close()
        B.close()


# ---- 10. a slab of a group --------------------------------------------------------------------------------

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
                s.set_average(["rho", "ux"], stride=2)
            assert e.value.code == L.IBLB_ERR_UNSUPPORTED
            msg = s._lib.iblb_last_error(s.handle)
            assert msg and len(msg.decode()) > 0
            assert s.average_info()["fields"] == 0
        group.step(2)
    finally:
        for s in slabs:
            s.close()
