"""iblb_get_fields on the GPU: every field on every kind of window against the numpy reference
(tests/fields_ref.py) applied to what the same context's iblb_get_macro and iblb_get_populations
return at that moment (both checked against the oracle elsewhere).

Lattices 24 x 37 and 16 x 130: odd heights, fewer than one wave and more than two waves of rows,
rows padded to whole waves; f64 and f32 storage.  State: seeded perturbed rho and u, a body force
with both components, five Lagrangian points (so the dense IB force is non-zero, one of them at the
x edge so that it is non-zero on both sides of the periodic wrap).  Read before the first step (boot
phase), after 1 step and after 9 (a deep launch plus remainders).

Tolerances.  rho, ux, uy: bit-equal to iblb_get_macro (the same arithmetic on the same
populations).  Vorticity: 64 * 2^-52 * max|u|; stress: 64 * 2^-52 * max rho: the rounding of a
9-term double sum taken in another order (the populations are O(rho), the velocity differences
O(max|u|)).  The same bounds hold for f32 storage: both sides start from the same doubles.
"""
import ctypes as C

import numpy as np
import pytest

import fields_ref as R
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W

pytestmark = pytest.mark.gpu

EPS = 64 * 2.0 ** -52
LATTICES = [(24, 37), (16, 130)]
PRECISIONS = ["f64", "f32"]
READS = [0, 1, 9]
BODY_FORCE = (1e-5, -2e-6)
ALL = list(R.NAMES)
LOCAL = [n for n in ALL if n != "vort"]


def points(nx, ny):
    """Five static points: inside the lattice, one at the x edge, one near each wall."""
    xs = np.array([0.4, 0.3 * nx, 0.5 * nx + 0.25, 0.7 * nx, nx - 1.3])
    ys = np.array([0.5 * ny, 1.2, 0.4 * ny + 0.5, ny - 2.4, 0.6 * ny])
    s = np.empty(10, dtype=np.float32)
    s[0::2], s[1::2] = xs, ys
    us = np.zeros(10, dtype=np.float32)
    us[0::2] = [1e-3, -5e-4, 8e-4, 3e-4, -1e-3]
    us[1::2] = [2e-4, 4e-4, -6e-4, 1e-4, 5e-4]
    return s, us, np.ones(5, dtype=np.int32)


def windows(nx, ny):
    return {
        "whole": None,
        "offset(1,1) stride(3,2)": (1, 1, (nx - 2) // 3 + 1, (ny - 2) // 2 + 1, 3, 2),
        "corner 0,0": (0, 0, 1, 1, 1, 1),
        "corner X,0": (nx - 1, 0, 1, 1, 1, 1),
        "corner 0,Y": (0, ny - 1, 1, 1, 1, 1),
        "corner X,Y": (nx - 1, ny - 1, 1, 1, 1, 1),
        "column 0": (0, 0, 1, ny, 1, 1),
        "column X": (nx - 1, 0, 1, ny, 1, 1),
        "row 0": (0, 0, nx, 1, 1, 1),
        "row Y": (0, ny - 1, nx, 1, 1, 1),
    }


def new_lattice(gpu, nx, ny, precision, with_points=True, **kw):
    rho, u = W.perturbed_state(nx, ny, 7)
    lat = gpu.Lattice(nx, ny, W.TAU, W.TAU2, precision=precision, body_force=BODY_FORCE,
                      max_points=8 if with_points else 0, **kw)
    lat.set_state(rho, u)
    if with_points:
        lat.set_lagrangian(*points(nx, ny))
    return lat


def check(got, ref, rho, u, names, what):
    """got / ref: {name: array}; the module's tolerances."""
    umax, rmax = np.max(np.abs(u)), np.max(rho)
    for n in names:
        g, r = got[n], ref[n]
        assert g.shape == r.shape, (what, n, g.shape, r.shape)
        if n in ("rho", "ux", "uy"):
            assert np.array_equal(g, r), (what, n, np.max(np.abs(g - r)))
        else:
            bound = EPS * (umax if n == "vort" else rmax)
            err = np.max(np.abs(g - r)) if g.size else 0.0
            assert err <= bound, (what, n, err, bound)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nx,ny", LATTICES)
def test_fields_match_the_reference_on_every_window(gpu, nx, ny, precision):
    lat = new_lattice(gpu, nx, ny, precision)
    try:
        done = 0
        for t in READS:
            if t > done:
                lat.step(t - done)
            done = t
            rho, u = lat.macro()
            full = R.fields_full(rho, u, lat.populations(), W.TAU, nx, ny)
            if t > 0:  # the state is not trivial: the stress is well above its tolerance
                assert np.max(np.abs(full["sxy"])) > 1e4 * EPS
            for name, w in windows(nx, ny).items():
                ref = {n: np.ascontiguousarray(R.sample(a, w)) for n, a in full.items()}
                i0, nxl = lat.window_local(w)
                assert (i0, nxl) == (0, nx if w is None else w[2])
                check(lat.fields(ALL, w), ref, rho, u, ALL, (nx, ny, precision, t, name))
            # a subset of the fields, given out of order: planes in ascending bit order
            sub = lat.fields(["sxy", "ux"], (1, 1, 2, 3, 3, 2))
            assert list(sub) == ["ux", "sxy"]
            check(sub, {n: R.sample(full[n], (1, 1, 2, 3, 3, 2)) for n in sub}, rho, u, list(sub), (t, "subset"))
    finally:
        lat.close()


def test_reading_does_not_disturb_the_run(gpu):
    nx, ny = LATTICES[0]
    a = new_lattice(gpu, nx, ny, "f64", with_points=False)
    b = new_lattice(gpu, nx, ny, "f64", with_points=False)
    try:
        a.step(3)
        a.fields(ALL)
        a.fields(ALL, (1, 1, (nx - 2) // 3 + 1, (ny - 2) // 2 + 1, 3, 2))
        a.step(6)
        b.step(9)
        assert np.array_equal(a.populations(), b.populations())
        ra, ua = a.macro()
        rb, ub = b.macro()
        assert np.array_equal(ra, rb) and np.array_equal(ua, ub)
    finally:
        a.close()
        b.close()


def slab_ref(slab, w):
    """fields_ref on the slab's own macro and populations, sampled on the slab's part of the
    global window w (the stress and the moments are local to a cell)."""
    rho, u = slab.macro()
    full = R.fields_full(rho, u, slab.populations(), W.TAU, slab.x_count, slab.ny)
    if w is None:
        w = (0, 0, slab.nx, slab.ny, 1, 1)
    x0, y0, wnx, wny, sx, sy = w
    xs = [x0 + i * sx for i in range(wnx) if slab.x_begin <= x0 + i * sx < slab.x_begin + slab.x_count]
    i_first = (xs[0] - x0) // sx if xs else None
    cols = np.array(xs, dtype=int) - slab.x_begin
    rows = y0 + sy * np.arange(wny)
    return {n: a[np.ix_(rows, cols)] for n, a in full.items()}, i_first, len(xs), rho, u


@pytest.mark.parametrize("precision", PRECISIONS)
def test_local_group_slabs(gpu, precision):
    nx, ny = LATTICES[0]
    rho, u = W.perturbed_state(nx, ny, 7)
    slabs = []
    for xb, xc in gpu.plan_slabs(nx, 3):
        s = gpu.Lattice(nx, ny, W.TAU, W.TAU2, precision=precision, body_force=BODY_FORCE, x_begin=xb, x_count=xc,
                        max_points=8)
        s.set_state(gpu.split_state(rho, 1, nx, ny, xb, xc), gpu.split_state(u, 2, nx, ny, xb, xc))
        s.set_lagrangian(*points(nx, ny))
        slabs.append(s)
    try:
        group = gpu.LocalGroup(slabs)
        inside = (9, 2, 3, 4, 2, 3)  # columns 9, 11, 13: the middle slab's only
        for t, n in ((0, 0), (9, 9)):
            if n:
                group.step(n)
            for name, w in (("whole", None), ("offset(1,1) stride(3,2)", (1, 1, 8, 18, 3, 2)), ("inside", inside)):
                parts = []
                for k, s in enumerate(slabs):
                    ref, i_first, nxl, r_s, u_s = slab_ref(s, w)
                    i0, n_loc = s.window_local(w)
                    assert n_loc == nxl and (nxl == 0 or i0 == i_first), (name, k, i0, n_loc, i_first, nxl)
                    got = s.fields(LOCAL, w)  # nx_local == 0: IBLB_OK and empty planes
                    check(got, ref, r_s, u_s, LOCAL, (precision, t, name, k))
                    parts.append(got)
                if name == "inside":
                    assert [p["rho"].shape[1] for p in parts] == [0, 3, 0]
                joined = group.fields(["rho", "sxy"], w)
                for n_ in ("rho", "sxy"):
                    assert np.array_equal(joined[n_], np.concatenate([p[n_] for p in parts], axis=1))
            # vorticity needs the neighbour slabs: refused with a message, the other fields still read
            for s in slabs:
                with pytest.raises(gpu.IblbError) as e:
                    s.fields(["vort"])
                assert e.value.code == L.IBLB_ERR_UNSUPPORTED
                msg = s._lib.iblb_last_error(s.handle)
                assert msg and len(msg.decode()) > 0
            with pytest.raises(gpu.IblbError) as e:
                group.fields(["ux", "vort"], inside)
            assert e.value.code == L.IBLB_ERR_UNSUPPORTED
    finally:
        for s in slabs:
            s.close()


def test_argument_errors_leave_the_context_usable(gpu):
    nx, ny = LATTICES[0]
    lat = new_lattice(gpu, nx, ny, "f64")
    try:
        lat.step(1)
        lib, h = lat._lib, lat.handle
        out = np.full(7 * nx * ny, -7.0)
        p = out.ctypes.data_as(C.c_void_p)
        ok = L.Window(0, 0, 2, 2, 1, 1)
        bad = {
            "sx = 0": (L.Window(0, 0, 2, 2, 0, 1), 1, p),
            "sy = 0": (L.Window(0, 0, 2, 2, 1, 0), 1, p),
            "nx = 0": (L.Window(0, 0, 0, 2, 1, 1), 1, p),
            "last sample at XDIM": (L.Window(nx - 1, 0, 2, 1, 1, 1), 1, p),
            "last sample at YDIM": (L.Window(0, ny - 2, 1, 2, 1, 2), 1, p),
            "negative x0": (L.Window(-1, 0, 2, 2, 1, 1), 1, p),
            "fields = 0": (ok, 0, p),
            "fields = 128": (ok, 128, p),
            "NULL out": (ok, 1, None),
        }
        for name, (w, fields, ptr) in bad.items():
            assert lib.iblb_get_fields(h, C.byref(w), fields, ptr) == L.IBLB_ERR_ARG, name
        assert np.all(out == -7.0)
        assert lib.iblb_window_local(h, C.byref(bad["sx = 0"][0]), None, None) == L.IBLB_ERR_ARG
        assert lib.iblb_window_local(h, C.byref(ok), None, None) == L.IBLB_OK
        with pytest.raises(ValueError):
            lat.fields(["pressure"])
        lat.step(2)
        rho, u = lat.macro()
        ref = R.fields_ref(rho, u, lat.populations(), W.TAU, nx, ny)
        check(lat.fields(ALL), ref, rho, u, ALL, "after the errors")
    finally:
        lat.close()
