"""The point-schedule scenarios (tests/point_schedule_cases.py) checked on the CPU, so that the GPU test
built on them (tests/test_gpu_point_schedules.py) can be trusted:

* every scenario's points_at agrees with its action list replayed through a small model of the contract of
  include/iblb.h (t0, the clamp to the last entry, the re-base at iblb_set_state, the points a checkpoint
  holds);
* the GPU test's tolerances cannot hide a wrong entry: the oracle run under a wrong mapping (every entry one
  iteration late; a schedule that wraps instead of holding its last entry; a schedule not re-based at a
  state reset) differs from the right one by at least 100 x the tolerance of either precision.
"""
import numpy as np
import pytest

import point_schedule_cases as C


@pytest.fixture(scope="module")
def cases():
    return C.scenarios()


def replay(actions, rebase=True, saved=None, g=0):
    """The contract in ten lines: the points every iteration of the action list uses, [(g, points)], and the
    (t, g, points) a "save" holds.  rebase False: iblb_set_state leaves t0 alone (entries before it clamp
    to entry 0), the behaviour before the re-base."""
    t, static, sched, t0, cur, used = 0, C.NONE, None, 0, C.NONE, []
    for a in actions:
        if a[0] == "schedule":
            ns = a[1].shape[1] // 2
            static, sched, t0 = (cur if ns else C.NONE), (a[1:] if ns else None), t
        elif a[0] == "points":
            static, sched = a[1:], None
        elif a[0] == "state":
            t, t0 = 0, (0 if rebase else t0)
        elif a[0] == "save":
            saved = (t, g, cur)
        elif a[0] == "load":
            (t, g, static), sched = saved, None
        elif a[0] == "step":
            for _ in range(a[1]):
                e = None if sched is None else min(max(t - t0, 0), len(sched[0]) - 1)
                cur = static if e is None else tuple(x[e] for x in sched)
                used.append((g, cur))
                t, g = t + 1, g + 1
    return used, saved


def same(p, q):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(p, q))


@pytest.mark.parametrize("name", list("ABCDEF"))
def test_points_at_matches_the_actions(cases, name):
    sc = cases[name]
    used, saved = replay(sc.actions)
    assert [g for g, _ in used] == list(range(sc.steps))
    for g, pts in used:
        assert same(pts, sc.points_at(g)), (name, g)
    assert (saved[1] if saved else None) == sc.saved_at
    for rname, acts in sc.restarts.items():
        got, _ = replay(acts, saved=saved)
        assert got and got[0][0] == sc.saved_at
        for g, pts in got:
            assert same(pts, sc.restart_points_at[rname](g)), (name, rname, g)


def test_scenario_shapes(cases):
    """What the scenarios are meant to exercise is there: calls that cut a schedule at offsets that are no
    multiple of K, exhaustion inside a call, a changing point count, entries that differ only in u_s and
    epsilon, a reset in mid-schedule, a checkpoint in mid-schedule."""
    K = C.K
    a, b, c, d, e, f = (cases[n] for n in "ABCDEF")
    assert a.steps == len(a.actions[0][1]) == 1 + 3 * K + 5 and b.steps <= a.steps
    assert len(b.actions[0][1]) == K + 3 < 1 + 2 * K  # exhausted inside the second call
    assert same(b.points_at(b.steps - 1), b.points_at(K + 2)) and not same(b.points_at(K + 1), b.points_at(K + 2))
    assert [p[0].size // 2 for p in (c.points_at(0), c.points_at(1 + K), c.points_at(2 * K + 3), c.points_at(c.steps - 1))] \
        == [120, 80, 0, 120]
    s0 = d.points_at(0)[0]
    flips = [g for g in range(1, d.steps) if not np.array_equal(d.points_at(g)[2], d.points_at(g - 1)[2])]
    assert all(np.array_equal(d.points_at(g)[0], s0) for g in range(d.steps)) and len(flips) == 1 and 1 < flips[0] < K
    assert all(not np.array_equal(d.points_at(g)[1], d.points_at(g - 1)[1]) for g in range(1, d.steps))
    assert e.resets == [2 * K + 3] and e.steps - e.resets[0] == 1 + 2 * K
    assert same(e.points_at(e.resets[0]), e.points_at(1 + K)) and not same(e.points_at(e.resets[0] - 1), e.points_at(e.resets[0]))
    assert f.saved_at == K + 3 and f.steps == 1 + 3 * K
    for sc in cases.values():  # every point inside the lattice, away from the x edge
        for g in range(sc.steps):
            s = sc.points_at(g)[0]
            assert s.size <= 2 * C.MAX_POINTS
            assert s.size == 0 or (s[0::2].min() > 30 and s[0::2].max() < C.NX - 30 and s[1::2].min() >= 1 and s[1::2].max() <= C.NY - 2)


def test_unrebased_model_is_the_old_behaviour(cases):
    """E's wrong mapping is what the model gives when iblb_set_state leaves the schedule's t0 alone."""
    e = cases["E"]
    used, _ = replay(e.actions, rebase=False)
    for g, pts in used:
        assert same(pts, e.wrong["not re-based"](g)), g


@pytest.mark.parametrize("name", list("ABCDEF"))
def test_flux_is_no_cancelled_remainder_where_it_is_compared(cases, oracle, name):
    """The GPU test's flux bound is relative to the oracle's cumulative flux.  That is meaningful only where
    the sum is not small against its own terms: at every iteration count at which the GPU test compares, the
    oracle's flux at C.FLUX_COLUMN is at least its largest term so far (the sums restart at a reset)."""
    sc = cases[name]
    runs = [(C.reference(oracle, sc, every=True), sc.compared)]
    for rname, acts in sc.restarts.items():
        end = sc.saved_at + sum(a[1] for a in acts if a[0] == "step")
        runs.append((C.oracle_run(oracle, sc.restart_points_at[rname], 0, end, marks=range(1, end + 1))[1], [end]))
    for snaps, compared in runs:
        for g in compared:
            g0 = max([r for r in sc.resets if r < g], default=0)
            flux = np.array([0.0] + [snaps[i]["flux"] for i in range(g0 + 1, g + 1)])
            terms = np.abs(np.diff(flux))
            print(name, g, "flux", flux[-1], "largest term", terms.max())
            assert abs(flux[-1]) >= terms.max(), (name, g, flux[-1], terms.max())


WRONG = [(n, w) for n, ws in (("A", ["late"]), ("B", ["late", "wrapped"]), ("C", ["late"]), ("D", ["late"]),
                              ("E", ["not re-based"])) for w in ws]


@pytest.mark.parametrize("name,wrong", WRONG)
def test_wrong_mapping_shows(cases, oracle, name, wrong):
    """Power: the oracle under the wrong mapping against the oracle under points_at, at the scenario's end,
    worst of rho, ux, uy each relative to its maximum, is at least 100 x the GPU test's field tolerance in
    f32 (1e-4, so 1e-2) and so in f64 (1e-10)."""
    sc = cases[name]
    assert list(sc.wrong) == [w for n, w in WRONG if n == name]
    good = C.reference(oracle, sc)[sc.steps]
    bad = C.reference(oracle, sc, sc.wrong[wrong])[sc.steps]
    n = C.NX * C.NY
    d = {"rho": C.rel(bad["rho"], good["rho"]), "ux": C.rel(bad["u"][:n], good["u"][:n]),
         "uy": C.rel(bad["u"][n:], good["u"][n:])}
    print(name, wrong, d)
    assert max(d.values()) >= 100 * max(C.FIELD_TOL.values()), (name, wrong, d)
