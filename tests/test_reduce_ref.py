"""combine_stats (cuda_iblb_11_amd/lattice.py) and the numpy reference of iblb_reduce_fields
(tests/reduce_ref.py), on the CPU: per-slab results merged in slab order must equal the reduction of the
whole window: counts, extrema and their locations exactly, every sum within the any-order summation
bound of reduce_ref."""
import math

import numpy as np
import pytest

import reduce_ref as R
from cuda_iblb_11_amd import Stats, combine_stats

NY, NX = 13, 17
# column ranges of the slabs: one slab, two, three, and three with an empty one in the middle
SPLITS = {"1": [(0, 17)], "2": [(0, 6), (6, 17)], "3": [(0, 5), (5, 11), (11, 17)], "3, one empty": [(0, 6), (6, 6), (6, 17)]}


def window():
    """Random samples with the extrema planted several times (ties within a row, across rows and
    across every split's slabs) and non-finite samples in different slabs."""
    a = np.random.default_rng(11).normal(size=(NY, NX))
    for j, i in ((7, 12), (7, 3), (2, 15), (9, 0)):  # first in row-major order: (2, 15)
        a[j, i] = -9.0
    for j, i in ((4, 16), (4, 5), (4, 6), (11, 1)):  # first: (4, 5)
        a[j, i] = 9.0
    a[0, 0] = a[6, 8] = np.nan
    a[12, 16] = np.inf
    a[3, 5] = -np.inf
    return a


def as_stats(r) -> Stats:
    return Stats(r.count, r.nonfinite, r.sum, r.sum_sq, r.min, r.max, r.min_i, r.min_j, r.max_i, r.max_j,
                 row_sum=np.array(r.row_sum), col_sum=np.array(r.col_sum))


def test_reference_on_a_known_window():
    r = R.reduce_one(window())
    assert (r.count, r.nonfinite) == (NY * NX - 4, 4)
    assert (r.min, r.min_i, r.min_j) == (-9.0, 15, 2) and (r.max, r.max_i, r.max_j) == (9.0, 5, 4)
    assert r.row_sum.shape == (NY,) and r.col_sum.shape == (NX,)
    a = np.where(np.isfinite(window()), window(), 0.0)
    assert np.allclose(r.row_sum, a.sum(axis=1)) and np.allclose(r.col_sum, a.sum(axis=0)) and np.isclose(r.sum, a.sum())
    e = R.reduce_one(np.full((3, 2), np.nan), i_first=4)
    assert (e.count, e.nonfinite, e.sum, e.min, e.max, e.min_i, e.max_j) == (0, 6, 0.0, math.inf, -math.inf, -1, -1)
    assert np.all(e.row_sum == 0) and np.all(e.col_sum == 0) and np.all(e.row_bound == 0)


def test_derived_quantities():
    rng = np.random.default_rng(3)
    f = {"rho": 1 + 1e-3 * rng.normal(size=(4, 5)), "ux": 1e-2 * rng.normal(size=(4, 5)), "uy": 1e-2 * rng.normal(size=(4, 5))}
    d = R.with_derived(f)
    for j in range(4):
        for i in range(5):
            r, ux, uy = (float(f[n][j, i]) for n in ("rho", "ux", "uy"))
            assert d["momx"][j, i] == r * ux and d["momy"][j, i] == r * uy
            assert d["usq"][j, i] == ux * ux + uy * uy and d["ke"][j, i] == 0.5 * (r * (ux * ux + uy * uy))


@pytest.mark.parametrize("split", list(SPLITS))
def test_combined_slabs_equal_the_whole(split):
    a = window()
    whole = R.reduce_one(a)
    parts = [as_stats(R.reduce_one(a[:, lo:hi], i_first=lo)) for lo, hi in SPLITS[split]]
    if "empty" in split:
        e = parts[1]
        assert e.count == 0 and e.min == math.inf and e.max == -math.inf and e.min_i == e.max_j == -1
        assert np.all(e.row_sum == 0) and e.col_sum.size == 0
    got = combine_stats(parts)
    R.check(got, whole, split)
    assert np.array_equal(got.col_sum, whole.col_sum)  # concatenated, not summed again
    # dicts of parts merge name by name; parts without row / column sums give none
    both = combine_stats([{"a": p, "b": p} for p in parts])
    assert list(both) == ["a", "b"] and both["b"].count == whole.count and both["b"].min_j == whole.min_j
    bare = combine_stats([Stats(p.count, p.nonfinite, p.sum, p.sum_sq, p.min, p.max, p.min_i, p.min_j, p.max_i, p.max_j)
                          for p in parts])
    R.check(bare, whole, split, rows=False, cols=False)


def test_ties_follow_row_major_order_whatever_the_slab_order_of_arrival():
    """The winner among equal extrema is the lowest j, then the lowest i, also when a later slab holds it."""
    lo = Stats(3, 0, 0.0, 0.0, -1.0, 2.0, 2, 5, 1, 5)
    hi = Stats(3, 0, 0.0, 0.0, -1.0, 2.0, 9, 4, 8, 5)
    c = combine_stats([lo, hi])
    assert (c.min_i, c.min_j) == (9, 4) and (c.max_i, c.max_j) == (1, 5)
    c = combine_stats([hi, lo])
    assert (c.min_i, c.min_j) == (9, 4) and (c.max_i, c.max_j) == (1, 5)
    with pytest.raises(ValueError):
        combine_stats([])
