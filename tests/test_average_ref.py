"""tests/average_ref.py (the numpy restatement the GPU tests compare with) against hand-made cases of
the definitions in include/iblb.h: iblb_set_average's sampling rule and the cuts of iblb_step."""
import numpy as np
import pytest

import average_ref as A


def sample(k):
    """Sample number k of a 2 x 3 window: exact small integers, different in every cell and sample."""
    base = np.arange(6, dtype=np.float64).reshape(2, 3)
    return {"rho": base + 10.0 * k, "ux": base - k, "uy": 2.0 * base + k}


def test_one_bin_adds_every_sample_in_order():
    s = [sample(k) for k in range(3)]
    (b,) = A.accumulate(s, 1, squares=True, uxuy=True)
    assert b["samples"] == 3 and list(b["sum"]) == ["rho", "ux", "uy"]
    for n in ("rho", "ux", "uy"):
        assert np.array_equal(b["sum"][n], s[0][n] + s[1][n] + s[2][n])
        assert np.array_equal(b["sum_sq"][n], s[0][n] ** 2 + s[1][n] ** 2 + s[2][n] ** 2)
    assert np.array_equal(b["sum_uxuy"], sum(x["ux"] * x["uy"] for x in s))
    # one cell by hand: cell (1, 2) holds 5; ux = 5, 4, 3; uy = 10, 11, 12
    assert b["sum"]["ux"][1, 2] == 12.0 and b["sum_sq"]["ux"][1, 2] == 50.0 and b["sum_uxuy"][1, 2] == 50 + 44 + 36


def test_sample_m_goes_to_bin_m_mod_nbins():
    s = [sample(k) for k in range(6)]
    bins = A.accumulate(s, 3)
    assert [b["samples"] for b in bins] == [2, 2, 2]
    for k, b in enumerate(bins):
        assert np.array_equal(b["sum"]["rho"], s[k]["rho"] + s[k + 3]["rho"])
        assert b["sum_sq"] is None and b["sum_uxuy"] is None


def test_counts_when_the_samples_are_no_multiple_of_nbins():
    s = [sample(k) for k in range(5)]
    bins = A.accumulate(s, 3)
    assert [b["samples"] for b in bins] == [2, 2, 1]
    assert np.array_equal(bins[2]["sum"]["uy"], s[2]["uy"])
    bins = A.accumulate(s[:2], 4, squares=True)
    assert [b["samples"] for b in bins] == [1, 1, 0, 0]
    assert not bins[3]["sum"]["rho"].any() and not bins[3]["sum_sq"]["rho"].any()


def test_the_sum_is_sequential_not_pairwise():
    # 1 + 2^-53 + 2^-53: added in sample order each half ulp is rounded away; any other order keeps one ulp
    one, h = np.ones((1, 1)), np.full((1, 1), 2.0 ** -53)
    (b,) = A.accumulate([{"ux": one}, {"ux": h}, {"ux": h}], 1)
    assert b["sum"]["ux"][0, 0] == 1.0
    (b,) = A.accumulate([{"ux": h}, {"ux": h}, {"ux": one}], 1)
    assert b["sum"]["ux"][0, 0] == 1.0 + 2.0 ** -52


def test_nothing_is_filtered():
    s = [sample(0), sample(1)]
    s[1]["ux"] = s[1]["ux"].copy()
    s[1]["ux"][0, 1] = np.nan
    (b,) = A.accumulate(s, 1, squares=True, uxuy=True)
    for plane in (b["sum"]["ux"], b["sum_sq"]["ux"], b["sum_uxuy"]):
        assert np.isnan(plane[0, 1]) and np.isfinite(np.delete(plane.ravel(), 1)).all()
    assert np.isfinite(b["sum"]["rho"]).all()


def test_bad_requests():
    with pytest.raises(ValueError):
        A.accumulate([{"ux": np.zeros((1, 1))}], 1, uxuy=True)
    with pytest.raises(ValueError):
        A.accumulate([sample(0)], 0)


def test_pieces_with_neither_set_are_the_calls():
    assert A.pieces([3, 4, 13], 2) == [(3, False, False), (4, False, False), (13, False, False)]


def test_pieces_of_one_event_set_count_on_across_calls():
    # averaging set at t0 = 2 with stride 5: samples after iterations 7, 12, 17, 22
    plan = A.pieces([3, 4, 13], 2, average=(2, 5))
    assert plan == [(3, False, False), (2, False, True), (2, False, False), (3, False, True), (5, False, True),
                    (5, False, True)]
    # the same as a tracer set
    assert A.pieces([3, 4, 13], 2, tracers=(2, 5)) == [(n, a, t) for n, t, a in plan]
    # set earlier than the state: the events already passed are not taken again
    assert A.pieces([4], 9, average=(2, 5)) == [(3, False, True), (1, False, False)]
    # stride 1: one piece per iteration; a stride longer than the calls: no event
    assert A.pieces([2], 0, average=(0, 1)) == [(1, False, True), (1, False, True)]
    assert A.pieces([3, 4], 0, average=(0, 8)) == [(3, False, False), (4, False, False)]


def test_pieces_cut_at_the_union_of_both_event_sets():
    # tracers every 3, averaging every 5 over step(17) from 0: events 3 5 6 9 10 12 15 (both) 17 (end)
    plan = A.pieces([17], 0, tracers=(0, 3), average=(0, 5))
    assert plan == [(3, True, False), (2, False, True), (1, True, False), (3, True, False), (1, False, True),
                    (2, True, False), (3, True, True), (2, False, False)]
    assert sum(p[0] for p in plan) == 17
    assert sum(p[1] for p in plan) == 5 and sum(p[2] for p in plan) == 3
    # different t0: tracers from 0, averaging from 2
    assert A.pieces([6], 2, tracers=(0, 4), average=(2, 3)) == [(2, True, False), (1, False, True), (3, True, True)]
