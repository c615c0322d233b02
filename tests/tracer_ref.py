"""numpy restatement of iblb_sample_points and of the tracer update rule (include/iblb.h), on arrays
shaped like Lattice.fields output: a field is an (ny, nx) array, field[y, x].

Every expression is written in the header's order with one numpy operation per arithmetic step, so
that each step is rounded once, as on the device (numpy's elementwise kernels do not contract a
multiply and an add): the results are meant to be compared with `==`.
"""
import numpy as np


def cells(x, y, nx, ny):
    """(i0, i1, j0, j1, a, b) of positions x, y (arrays) on an nx x ny lattice."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    fx = np.floor(x)
    i0 = fx.astype(np.int64)
    i1 = (i0 + 1) % nx
    a = x - fx
    j0 = np.minimum(np.floor(y).astype(np.int64), ny - 2)
    j1 = j0 + 1
    b = y - j0.astype(np.float64)
    return i0, i1, j0, j1, a, b


def sample(field, x, y):
    """Bilinear sample of one (ny, nx) field at the points (x, y): periodic in x, b = 1 on the top row."""
    field = np.asarray(field, dtype=np.float64)
    ny, nx = field.shape
    i0, i1, j0, j1, a, b = cells(x, y, nx, ny)
    v00, v10, v01, v11 = field[j0, i0], field[j0, i1], field[j1, i0], field[j1, i1]
    with np.errstate(invalid="ignore", over="ignore"):
        return (1.0 - b) * ((1.0 - a) * v00 + a * v10) + b * ((1.0 - a) * v01 + a * v11)


def sample_fields(fields, x, y):
    """{name: (ny, nx) array} -> {name: [n] array}."""
    return {n: sample(f, x, y) for n, f in fields.items()}


def advect(ux, uy, x, y, laps, stride):
    """One update of the tracers (x, y, laps) over `stride` iterations in the velocity fields ux, uy
    ((ny, nx) arrays) held fixed.  Returns new (x, y, laps); the inputs are left unchanged."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    laps = np.asarray(laps, dtype=np.int32)
    ny, nx = np.asarray(ux).shape
    X, ytop, s = float(nx), float(ny - 1), float(stride)
    su, sv = sample(ux, x, y), sample(uy, x, y)
    ok = np.isfinite(su) & np.isfinite(sv)
    with np.errstate(invalid="ignore", over="ignore"):
        xn = x + s * su
        yn = y + s * sv
        up, down = xn >= X, xn < 0.0
        xw = np.where(up, xn - X, np.where(down, xn + X, xn))
        lw = laps + up.astype(np.int32) - down.astype(np.int32)
        moved = ok & (xw >= 0.0) & (xw < X)  # else: more than one lattice length, or a non-finite u
        yc = np.where(yn < 0.0, 0.0, np.where(yn > ytop, ytop, yn))
    return np.where(moved, xw, x), np.where(ok, yc, y), np.where(moved, lw, laps).astype(np.int32)


def special_points(nx, ny):
    """Positions where the definition has an edge: cell centres (weights exactly 0 and 1), the
    periodic column pair (XDIM-1, 0), the top row (b = 1), the corners and the last representable
    position below XDIM."""
    below = np.nextafter(float(nx), 0.0)
    pts = [
        (0.0, 0.0), (3.0, 2.0), (float(nx - 1), 0.0), (0.0, float(ny - 1)), (float(nx - 1), float(ny - 1)),
        (nx - 1 + 0.25, 1.5), (nx - 0.5, ny - 1.0), (below, 0.75), (below, float(ny - 1)),
        (2.5, float(ny - 1)), (2.5, ny - 1.5), (2.5, float(ny - 2)), (0.5, 0.5), (nx / 2 + 0.125, ny / 2 - 0.375),
    ]
    return np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
