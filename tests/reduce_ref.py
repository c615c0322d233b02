"""TEST INFRASTRUCTURE: numpy reference of iblb_reduce_fields (include/iblb.h).

`reduce_ref(fields, i_first)` takes a {name: array (ny, nx)} dict as Lattice.fields returns it (this
slab's samples of a window, sample column 0 being window index i_first) and returns, per name, what
the reduction must give:

  count, nonfinite        finite / non-finite samples
  min, max                over the finite samples (+inf / -inf when there is none), and
  min_i, min_j, ...       the first such sample in row-major order (numpy's argmin / argmax; -1 when none)
  sum, sum_sq             math.fsum (the correctly rounded exact sum) of the finite x and x*x
  row_sum, col_sum        the same per window row / per sample column

together with the any-order summation bound of each sum: a sum of n doubles taken in any order is
within gamma_{n-1} * sum|x| < n * 2^-53 * sum|x| of the exact sum (Higham, Accuracy and Stability of
Numerical Algorithms, §4.2).  The squares x*x are single products, rounded alike on both sides, so
the bound of sum_sq is the same with x*x for |x|.

`with_derived(fields)` adds the four reduce-only quantities from rho, ux, uy in the stated order of
operations (one rounding each, as numpy evaluates them).
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

NAMES = ("rho", "ux", "uy", "vort", "sxx", "sxy", "syy", "momx", "momy", "ke", "usq")
DERIVED = ("momx", "momy", "ke", "usq")
U = 2.0 ** -53


def with_derived(fields: dict) -> dict:
    """fields plus momx = rho*ux, momy = rho*uy, ke = 0.5*(rho*(ux*ux + uy*uy)), usq = ux*ux + uy*uy."""
    out = dict(fields)
    with np.errstate(all="ignore"):
        rho, ux, uy = fields["rho"], fields["ux"], fields["uy"]
        out["momx"] = rho * ux
        out["momy"] = rho * uy
        out["ke"] = 0.5 * (rho * (ux * ux + uy * uy))
        out["usq"] = ux * ux + uy * uy
    return out


def _sums(x: np.ndarray, fin: np.ndarray, axis):
    """(fsum, bound) of the finite entries of x: over everything (axis None), per row (axis 1) or per
    column (axis 0)."""
    def one(v, m):
        v = v[m]
        return math.fsum(v), v.size * U * math.fsum(np.abs(v))
    if axis is None:
        return one(x.ravel(), fin.ravel())
    lines = x if axis == 1 else x.T
    masks = fin if axis == 1 else fin.T
    pairs = [one(v, m) for v, m in zip(lines, masks)]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


def reduce_one(a: np.ndarray, i_first: int = 0) -> SimpleNamespace:
    a = np.asarray(a, dtype=np.float64)
    ny, nx = a.shape
    fin = np.isfinite(a)
    r = SimpleNamespace(count=int(fin.sum()), nonfinite=int(a.size - fin.sum()))
    with np.errstate(all="ignore"):
        sq = a * a
    r.sum, r.sum_bound = _sums(a, fin, None)
    r.sum_sq, r.sum_sq_bound = _sums(sq, fin, None)
    r.row_sum, r.row_bound = _sums(a, fin, 1) if nx else (np.zeros(ny), np.zeros(ny))
    r.col_sum, r.col_bound = _sums(a, fin, 0) if nx else (np.zeros(0), np.zeros(0))
    if r.count:
        jlo, ilo = np.unravel_index(np.argmin(np.where(fin, a, np.inf)), a.shape)
        jhi, ihi = np.unravel_index(np.argmax(np.where(fin, a, -np.inf)), a.shape)
        r.min, r.max = float(a[jlo, ilo]), float(a[jhi, ihi])
        r.min_i, r.min_j, r.max_i, r.max_j = int(ilo) + i_first, int(jlo), int(ihi) + i_first, int(jhi)
    else:
        r.min, r.max = math.inf, -math.inf
        r.min_i = r.min_j = r.max_i = r.max_j = -1
    return r


def reduce_ref(fields: dict, i_first: int = 0) -> dict:
    return {n: reduce_one(a, i_first) for n, a in fields.items()}


def check(got, ref, what, rows=True, cols=True) -> None:
    """got: a Stats of the package; ref: reduce_one's result.  Counts, extrema and their locations
    exact; every sum within its bound."""
    for f in ("count", "nonfinite", "min_i", "min_j", "max_i", "max_j"):
        assert getattr(got, f) == getattr(ref, f), (what, f, getattr(got, f), getattr(ref, f))
    assert got.min == ref.min and got.max == ref.max, (what, got.min, ref.min, got.max, ref.max)
    assert abs(got.sum - ref.sum) <= ref.sum_bound, (what, "sum", got.sum, ref.sum, ref.sum_bound)
    assert abs(got.sum_sq - ref.sum_sq) <= ref.sum_sq_bound, (what, "sum_sq", got.sum_sq, ref.sum_sq, ref.sum_sq_bound)
    for on, g, r, b in ((rows, got.row_sum, ref.row_sum, ref.row_bound), (cols, got.col_sum, ref.col_sum, ref.col_bound)):
        if on:
            assert g is not None and g.shape == r.shape, (what, None if g is None else g.shape, r.shape)
            assert np.all(np.abs(g - r) <= b), (what, "row / column sums", float(np.max(np.abs(g - r) - b)))
        else:
            assert g is None, what
