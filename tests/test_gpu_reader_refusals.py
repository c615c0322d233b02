"""Refused calls of the readers and in-step observers: the return code and the whole iblb_last_error text of
each, the order of the argument checks, and that a refusal leaves the context as it was.

A 64 x 32 lone slab, f64 and f32 storage, the same rows for both.  The expected texts are copied from the
sources of the C ABI (csrc/): they are what a caller's logs and tests match, so moving a reader must not
change them.  Every row goes through the ctypes functions, not through Lattice, whose own argument checks
would raise first.  After every refusal iblb_get_macro returns what it returned before, bit for bit.

The refusals that need a group (vorticity, iblb_sample_points, iblb_set_tracers and iblb_set_average on a
slab, iblb_gather_macro on a local group) are asserted by the group tests (test_gpu_fields.py,
test_gpu_reduce.py, test_gpu_tracers.py, test_gpu_average.py, test_gpu_group_readers.py).
"""
import ctypes as C

import numpy as np
import pytest

from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_fields import BODY_FORCE
from test_gpu_tracers import new_lattice

pytestmark = pytest.mark.gpu

NX, NY = 64, 32
PRECISIONS = ["f64", "f32"]
RHO, UX, UY, VORT = (L.FIELDS[n] for n in ("rho", "ux", "uy", "vort"))
ARG, STATE = L.IBLB_ERR_ARG, L.IBLB_ERR_STATE

NO_STATE = "no state: call iblb_set_state first"
BAD_FIELDS = "fields: no field or an unknown IBLB_FIELD_* bit"
BAD_QUANTITIES = "fields: no quantity or an unknown IBLB_FIELD_* / IBLB_QTY_* bit"
BAD_WINDOW = "window: need sx, sy, nx, ny >= 1 and every sample inside the lattice (no wrap)"
BAD_POINT = "point %d is non-finite or outside 0 <= x < XDIM, 0 <= y <= YDIM-1"

# scratch the refused calls may be handed (none of them writes it)
OUT = np.zeros(11 * NX * NY)
STATS = (L.FieldStats * 11)()
PX, PY = np.array([3.5, 10.0, 20.25]), np.array([2.0, 7.5, 30.0])


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def win(x0=0, y0=0, nx=NX, ny=NY, sx=1, sy=1):
    return C.byref(L.Window(x0, y0, nx, ny, sx, sy))


def stride_zero():
    return win(sx=0)


def past_x():
    return win(x0=1)  # the last sample is column NX


def past_y():
    return win(ny=NY // 2 + 1, sy=2)  # the last sample is row NY


def xy(x=None, y=None):
    return ptr(PX if x is None else np.array(x, dtype=float)), ptr(PY if y is None else np.array(y, dtype=float))


def with_average(call, fields=RHO | UX | UY, nbins=2, flags=0):
    """The refused call on a context that averages `fields`."""
    def row(lib, h):
        assert lib.iblb_set_average(h, None, fields, 4, nbins, flags) == L.IBLB_OK
        return call(lib, h)
    return row


# every reader that needs a state, called before iblb_set_state
READERS = [
    ("get_macro", lambda lib, h: lib.iblb_get_macro(h, ptr(OUT), ptr(OUT))),
    ("get_populations", lambda lib, h: lib.iblb_get_populations(h, ptr(OUT))),
    ("get_force", lambda lib, h: lib.iblb_get_force(h, ptr(OUT))),
    ("get_lagrangian_force", lambda lib, h: lib.iblb_get_lagrangian_force(h, ptr(OUT))),
    ("get_flux", lambda lib, h: lib.iblb_get_flux(h, C.byref(C.c_double(0.)))),
    ("count_nonfinite", lambda lib, h: lib.iblb_count_nonfinite(h, C.byref(C.c_longlong(0)))),
    ("get_fields", lambda lib, h: lib.iblb_get_fields(h, None, RHO, ptr(OUT))),
    ("reduce_fields", lambda lib, h: lib.iblb_reduce_fields(h, None, RHO, STATS, None, None)),
    ("sample_points", lambda lib, h: lib.iblb_sample_points(h, 3, *xy(), RHO, ptr(OUT))),
    ("gather_macro", lambda lib, h: lib.iblb_gather_macro(h, 0, ptr(OUT), ptr(OUT))),
]

# (id, call, return code, iblb_last_error) on a context with a state, three iterations on
ROWS = [
    # -- the field bits
    ("get_fields-no-field", lambda lib, h: lib.iblb_get_fields(h, None, 0, ptr(OUT)), ARG, BAD_FIELDS),
    ("get_fields-unknown-bit", lambda lib, h: lib.iblb_get_fields(h, None, RHO | 128, ptr(OUT)), ARG, BAD_FIELDS),
    ("reduce_fields-no-field", lambda lib, h: lib.iblb_reduce_fields(h, None, 0, STATS, None, None), ARG,
     BAD_QUANTITIES),
    ("reduce_fields-unknown-bit", lambda lib, h: lib.iblb_reduce_fields(h, None, RHO | 2048, STATS, None, None), ARG,
     BAD_QUANTITIES),
    ("sample_points-no-field", lambda lib, h: lib.iblb_sample_points(h, 3, *xy(), 0, ptr(OUT)), ARG, BAD_FIELDS),
    ("sample_points-unknown-bit", lambda lib, h: lib.iblb_sample_points(h, 3, *xy(), UX | 128, ptr(OUT)), ARG,
     BAD_FIELDS),
    ("set_average-no-field", lambda lib, h: lib.iblb_set_average(h, win(), 0, 1, 1, 0), ARG, BAD_FIELDS),
    ("set_average-unknown-bit", lambda lib, h: lib.iblb_set_average(h, None, RHO | 128, 1, 1, 0), ARG, BAD_FIELDS),
    # -- the window
    ("get_fields-sx-zero", lambda lib, h: lib.iblb_get_fields(h, stride_zero(), RHO, ptr(OUT)), ARG, BAD_WINDOW),
    ("get_fields-past-x", lambda lib, h: lib.iblb_get_fields(h, past_x(), RHO, ptr(OUT)), ARG, BAD_WINDOW),
    ("get_fields-past-y", lambda lib, h: lib.iblb_get_fields(h, past_y(), RHO, ptr(OUT)), ARG, BAD_WINDOW),
    ("reduce_fields-sx-zero", lambda lib, h: lib.iblb_reduce_fields(h, stride_zero(), RHO, STATS, None, None), ARG,
     BAD_WINDOW),
    ("reduce_fields-past-x", lambda lib, h: lib.iblb_reduce_fields(h, past_x(), RHO, STATS, None, None), ARG,
     BAD_WINDOW),
    ("window_local-sx-zero", lambda lib, h: lib.iblb_window_local(h, stride_zero(), None, None), ARG, BAD_WINDOW),
    ("window_local-past-x", lambda lib, h: lib.iblb_window_local(h, past_x(), None, None), ARG, BAD_WINDOW),
    ("set_average-sx-zero", lambda lib, h: lib.iblb_set_average(h, stride_zero(), RHO, 1, 1, 0), ARG, BAD_WINDOW),
    ("set_average-past-x", lambda lib, h: lib.iblb_set_average(h, past_x(), RHO, 1, 1, 0), ARG, BAD_WINDOW),
    # -- the destinations
    ("get_fields-out-null", lambda lib, h: lib.iblb_get_fields(h, None, RHO, None), ARG, "out is NULL"),
    ("reduce_fields-stats-null", lambda lib, h: lib.iblb_reduce_fields(h, None, RHO, None, None, None), ARG,
     "stats is NULL"),
    # -- points
    ("sample_points-n-negative", lambda lib, h: lib.iblb_sample_points(h, -1, *xy(), RHO, ptr(OUT)), ARG,
     "n is negative"),
    ("sample_points-null", lambda lib, h: lib.iblb_sample_points(h, 3, *xy(), RHO, None), ARG, "x, y or out is NULL"),
    ("sample_points-nan", lambda lib, h: lib.iblb_sample_points(h, 3, *xy(y=[2.0, float("nan"), 30.0]), RHO, ptr(OUT)),
     ARG, BAD_POINT % 1),
    ("sample_points-x-is-xdim", lambda lib, h: lib.iblb_sample_points(h, 3, *xy(x=[3.5, 10.0, float(NX)]), RHO, ptr(OUT)),
     ARG, BAD_POINT % 2),
    ("set_tracers-n-negative", lambda lib, h: lib.iblb_set_tracers(h, -1, *xy(), 1), ARG, "n is negative"),
    ("set_tracers-stride-zero", lambda lib, h: lib.iblb_set_tracers(h, 3, *xy(), 0), ARG, "stride must be >= 1"),
    ("set_tracers-null", lambda lib, h: lib.iblb_set_tracers(h, 3, xy()[0], None, 1), ARG, "x or y is NULL"),
    ("set_tracers-y-above-the-wall", lambda lib, h: lib.iblb_set_tracers(h, 3, *xy(y=[float(NY), 7.5, 30.0]), 1), ARG,
     BAD_POINT % 0),
    # -- averaging
    ("set_average-uxuy-without-ux", lambda lib, h: lib.iblb_set_average(h, None, RHO | UY, 1, 1, L.AVG_UXUY), ARG,
     "IBLB_AVG_UXUY needs both IBLB_FIELD_UX and IBLB_FIELD_UY"),
    ("set_average-stride-zero", lambda lib, h: lib.iblb_set_average(h, None, RHO, 0, 1, 0), ARG, "stride must be >= 1"),
    ("set_average-nbins-zero", lambda lib, h: lib.iblb_set_average(h, None, RHO, 1, 0, 0), ARG, "nbins must be >= 1"),
    ("set_average-unknown-flag", lambda lib, h: lib.iblb_set_average(h, None, RHO, 1, 1, 4), ARG,
     "flags: an unknown IBLB_AVG_* bit"),
    ("get_average-nothing-set", lambda lib, h: lib.iblb_get_average(h, 0, ptr(OUT), None, None, None), STATE,
     "iblb_get_average: no averaging is set"),
    ("reset_average-nothing-set", lambda lib, h: lib.iblb_reset_average(h), STATE,
     "iblb_reset_average: no averaging is set"),
    ("get_average-bin-is-nbins", with_average(lambda lib, h: lib.iblb_get_average(h, 2, ptr(OUT), None, None, None)), ARG,
     "bin is outside [0, nbins)"),
    ("get_average-bin-negative", with_average(lambda lib, h: lib.iblb_get_average(h, -1, ptr(OUT), None, None, None)), ARG,
     "bin is outside [0, nbins)"),
    ("get_average-sum_sq-not-requested",
     with_average(lambda lib, h: lib.iblb_get_average(h, 0, ptr(OUT), ptr(OUT), None, None), flags=L.AVG_UXUY), ARG,
     "sum_sq was not requested (IBLB_AVG_SQ)"),
    ("get_average-sum_uxuy-not-requested",
     with_average(lambda lib, h: lib.iblb_get_average(h, 0, ptr(OUT), None, ptr(OUT), None), flags=L.AVG_SQ), ARG,
     "sum_uxuy was not requested (IBLB_AVG_UXUY)"),
    # -- the order of the checks: two faults, the earlier message
    ("order-get_fields-bits-before-window", lambda lib, h: lib.iblb_get_fields(h, stride_zero(), 128, ptr(OUT)), ARG,
     BAD_FIELDS),
    ("order-reduce_fields-bits-before-window", lambda lib, h: lib.iblb_reduce_fields(h, past_x(), 0, STATS, None, None),
     ARG, BAD_QUANTITIES),
    ("order-get_fields-window-before-out", lambda lib, h: lib.iblb_get_fields(h, past_x(), RHO, None), ARG, BAD_WINDOW),
    ("order-get_fields-out-before-vorticity", lambda lib, h: lib.iblb_get_fields(h, None, VORT, None), ARG, "out is NULL"),
    ("order-reduce_fields-stats-before-vorticity", lambda lib, h: lib.iblb_reduce_fields(h, None, VORT, None, None, None),
     ARG, "stats is NULL"),
    ("order-sample_points-n-before-bits", lambda lib, h: lib.iblb_sample_points(h, -1, *xy(), 0, ptr(OUT)), ARG,
     "n is negative"),
    ("order-sample_points-bits-before-positions",
     lambda lib, h: lib.iblb_sample_points(h, 3, *xy(x=[-1.0, 10.0, 20.0]), 0, ptr(OUT)), ARG, BAD_FIELDS),
    ("order-set_average-bits-before-flags", lambda lib, h: lib.iblb_set_average(h, None, 128, 1, 1, 4), ARG, BAD_FIELDS),
    ("order-set_average-flags-before-window", lambda lib, h: lib.iblb_set_average(h, stride_zero(), RHO, 1, 1, 4), ARG,
     "flags: an unknown IBLB_AVG_* bit"),
    ("order-set_tracers-n-before-stride", lambda lib, h: lib.iblb_set_tracers(h, -1, *xy(), 0), ARG, "n is negative"),
]


def last_error(lib, h):
    return lib.iblb_last_error(h).decode()


def macro(lib, h):
    rho, u = np.empty(NX * NY), np.empty(2 * NX * NY)
    assert lib.iblb_get_macro(h, ptr(rho), ptr(u)) == L.IBLB_OK
    return rho, u


@pytest.fixture(scope="module", params=PRECISIONS)
def ready(request, gpu):
    """One lattice per precision for every row: its state three iterations on, and that state's macro."""
    lat = new_lattice(gpu, NX, NY, request.param)
    lat.step(3)
    yield lat, macro(lat._lib, lat.handle)
    lat.close()


@pytest.mark.parametrize("name,call,code,text", ROWS, ids=[r[0] for r in ROWS])
def test_refusal(ready, name, call, code, text):
    lat, (rho, u) = ready
    lib, h = lat._lib, lat.handle
    try:
        assert call(lib, h) == code
        assert last_error(lib, h) == text
    finally:  # rows that installed an average remove it
        assert lib.iblb_set_average(h, None, 0, 1, 1, 0) == L.IBLB_OK
    # nothing was installed, nothing moved
    assert lat.tracer_info()["n"] == 0 and lat.average_info()["fields"] == 0 and lat.steps == 3
    r, v = macro(lib, h)
    assert np.array_equal(r, rho) and np.array_equal(v, u)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_readers_before_set_state(gpu, precision):
    """Every reader refuses a context without a state; the state set afterwards reads like a fresh lattice's."""
    fresh = new_lattice(gpu, NX, NY, precision)
    lat = gpu.Lattice(NX, NY, W.TAU, W.TAU2, precision=precision, body_force=BODY_FORCE)
    try:
        lib, h = lat._lib, lat.handle
        for name, call in READERS:
            assert call(lib, h) == STATE, name
            assert last_error(lib, h) == NO_STATE, name
        rho, u = W.perturbed_state(NX, NY, 7)  # new_lattice's state
        lat.set_state(rho, u)
        for got, want in zip(macro(lib, h), macro(fresh._lib, fresh.handle)):
            assert np.array_equal(got, want)
    finally:
        lat.close()
        fresh.close()
