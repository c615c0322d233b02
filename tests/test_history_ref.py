"""tests/history_ref.py checked on the CPU: the ring's slot arithmetic against a plain list of records, the
statistics against a scalar loop in Python floats, and the cases the GPU tests lean on shown not to be vacuous."""
import math

import numpy as np
import pytest

import history_ref as H
import tracer_ref as T


def series(n_rec, planes=2, n=3, seed=5):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n_rec, planes, n))


@pytest.mark.parametrize("capacity", [1, 3, 8, 20])
def test_the_ring_returns_the_last_capacity_records(capacity):
    recs = series(8)
    h = H.History(2, 3, capacity)
    for m, r in enumerate(recs):
        h.append(r, 10 + 5 * m)
        oldest = max(0, m + 1 - capacity)
        got, it = h.get()
        assert np.array_equal(got, recs[oldest:m + 1])
        assert np.array_equal(it, 10 + 5 * np.arange(oldest, m + 1))
        assert H.window(m + 1, capacity) == (oldest, m + 1)
    # every stretch inside the window, and no stretch outside it
    oldest = max(0, 8 - capacity)
    for first in range(-1, 10):
        for count in range(-1, 10):
            ok = count >= 0 and first >= oldest and first + count <= 8
            assert H.readable(first, count, 8, capacity) == ok
            if ok:
                assert np.array_equal(h.get(first, count)[0], recs[first:first + count])
                rr = H.runs(first, count, capacity)
                assert len(rr) <= 2 and sum(n for _, n in rr) == count
                assert all(0 <= s and s + n <= capacity for s, n in rr)
            else:
                with pytest.raises(ValueError):
                    h.get(first, count)


def test_a_wrapped_ring_differs_from_an_unwrapped_one():
    recs = series(8)
    small, large = H.History(2, 3, 3), H.History(2, 3, 16)
    for m, r in enumerate(recs):
        small.append(r, m)
        large.append(r, m)
    a, b = small.get()[0], large.get()[0]
    assert a.shape[0] == 3 and b.shape[0] == 8
    assert not np.array_equal(a, b[:3])  # the slots were overwritten: not the first three records
    assert np.array_equal(a, b[5:])
    assert H.slot(7, 3) == 1 and H.runs(5, 3, 3) == [(2, 1), (0, 2)]
    for k in H.STAT_KEYS:  # the statistics do not depend on the ring's size
        assert np.array_equal(small.stats[k], large.stats[k]), k


def test_the_statistics_equal_a_scalar_loop():
    recs = series(9, planes=2, n=4, seed=9)
    recs[3, 0, 1] = np.nan
    recs[5, 1, 2] = np.inf
    h = H.History(2, 4, 2)
    for m, r in enumerate(recs):
        h.append(r, m)
    for k in range(2):
        for p in range(4):
            cnt = nonf = 0
            s = sq = 0.0
            lo, hi, lo_m, hi_m = math.inf, -math.inf, -1, -1
            for m in range(9):
                v = float(recs[m, k, p])
                if not math.isfinite(v):
                    nonf += 1
                    continue
                cnt += 1
                s = s + v
                sq = sq + v * v
                if v < lo:
                    lo, lo_m = v, m
                if v > hi:
                    hi, hi_m = v, m
            got = tuple(h.stats[key][k, p] for key in H.STAT_KEYS)
            assert got == (cnt, nonf, s, sq, lo, hi, lo_m, hi_m), (k, p)
    assert h.stats["nonfinite"].sum() == 2


def test_a_maximum_in_an_overwritten_record_is_still_reported():
    v = np.array([0.5, 9.0, 0.25, -1.0, 0.75, 0.125]).reshape(6, 1, 1)
    h = H.History(1, 1, 2)
    for m, r in enumerate(v):
        h.append(r, m)
    held = h.get()[0]
    assert held.max() < 9.0 and H.window(6, 2) == (4, 6)
    assert h.stats["max"][0, 0] == 9.0 and h.stats["max_rec"][0, 0] == 1  # record 1 is gone from the ring
    assert h.stats["min"][0, 0] == -1.0 and h.stats["min_rec"][0, 0] == 3
    assert h.stats["count"][0, 0] == 6


def test_a_nan_sample_moves_only_nonfinite():
    h = H.History(1, 2, 4)
    h.append(np.array([[1.0, 2.0]]), 0)
    before = {k: a.copy() for k, a in h.stats.items()}
    h.append(np.array([[np.nan, 3.0]]), 1)
    for k in H.STAT_KEYS:
        if k == "nonfinite":
            assert h.stats[k][0, 0] == before[k][0, 0] + 1
        else:
            assert h.stats[k][0, 0] == before[k][0, 0], k
    assert h.stats["count"][0, 1] == 2 and h.stats["max_rec"][0, 1] == 1 and h.stats["nonfinite"][0, 1] == 0
    assert np.isnan(h.get()[0][1, 0, 0])  # the ring holds the sample as it was


def test_nothing_seen_and_reset():
    h = H.History(2, 2, 3)
    assert np.all(h.stats["min"] == np.inf) and np.all(h.stats["max"] == -np.inf)
    assert np.all(h.stats["min_rec"] == -1) and np.all(h.stats["max_rec"] == -1)
    assert h.get()[0].shape == (0, 2, 2)
    h.append(np.ones((2, 2)), 4)
    h.reset()
    assert h.recorded == 0 and np.all(h.stats["count"] == 0) and np.all(h.stats["min"] == np.inf)
    assert h.get()[0].shape == (0, 2, 2)


def test_a_record_of_fields_is_the_point_sample():
    rng = np.random.default_rng(2)
    nx, ny = 7, 5
    fields = {"ux": rng.normal(size=(ny, nx)), "uy": rng.normal(size=(ny, nx))}
    x, y = T.special_points(nx, ny)
    r = H.record_of(fields, ["ux", "uy"], x, y)
    assert r.shape == (2, x.size)
    assert np.array_equal(r[0], T.sample(fields["ux"], x, y)) and np.array_equal(r[1], T.sample(fields["uy"], x, y))
