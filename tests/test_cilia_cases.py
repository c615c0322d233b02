"""The on-device cilia scenarios (tests/cilia_cases.py) checked on the CPU with the oracle alone, so that the
GPU tests built on them (tests/test_gpu_cilia_paths.py, tests/mock_rccl/run_cilia.py) can be trusted:

* every case stays inside its configuration's horizon, counted from the last state reset, and the unseeded
  twin's max|u| is <= 0.03 at the end of every case: no case sits on the blow-up of the reference's penalty
  IB.  The 0.03 is a condition, not a measurement;
* the GPU tests' tolerances cannot hide a sequencing error of the kinematics.  Three are seeded into the twin:
  `it` off by one, a fresh Cilia (zeroed `lasts`) at the hand-over between two calls of case 1, no restart
  of the beat at the state reset of case 2.  Each moves rho, u_x or u_y, in the GPU test's own measure (each
  relative to its maximum), by at least 1e-3: 1000 x the f64 bound (1e-9) and 10 x the f32 bound (1e-4);
* the fields are the detector, not the points: after the zeroed `lasts` the points and u_s at the end of the
  run are bit-identical to the unseeded twin's, so a comparison of lagrangian() alone would pass.
"""
import numpy as np
import pytest

import cilia_cases as CC

K = CC.K
POWER = 1e-3
assert POWER >= 1000 * CC.FIELD_TOL["f64"] and POWER >= 10 * CC.FIELD_TOL["f32"]

RCCL_CALLS = {"WIDE": [(1, 12, 3, 5), (1, 2, 3, 2, 4)], "REF": [(1, 5, 7)]}


def all_cases():
    W, R = CC.WIDE, CC.REF
    out = [("case1 depth 4", W, CC.case1(4)), ("case1 depth 5, 22 iterations", W, CC.case1(5)[:4]),
           ("case2 WIDE", W, CC.CASE2_WIDE), ("case2 REF", R, CC.CASE2_REF),
           ("case4", W, CC.steps(CC.CASE4_STEPS)), ("case5", W, CC.case5()), ("case6", R, CC.CASE6),
           ("group WIDE", W, CC.steps(*CC.GROUP_CALLS)), ("group REF", R, CC.steps(*CC.GROUP_CALLS))]
    out += [("case3 " + n, W, CC.steps(*c)) for n, c in CC.CASE3.items()]
    out += [(f"rccl {n} {c}", CC.CONFIGS[n], CC.steps(*c)) for n, cs in RCCL_CALLS.items() for c in cs]
    return out


def moved(bad, good):
    d = CC.fields_rel(bad["rho"], bad["u"], good["rho"], good["u"])
    return d, max(d["rho"], d["ux"], d["uy"])


@pytest.mark.parametrize("name,cfg,actions", all_cases(), ids=[c[0] for c in all_cases()])
def test_cases_stay_off_the_blow_up(oracle, name, cfg, actions):
    longest, n = CC.total(actions)
    assert longest <= cfg.horizon, (name, longest, cfg.horizon)
    tw, snaps = CC.run_twin(oracle, cfg, actions)
    assert tw.g == n
    worst = max(float(np.max(np.abs(s["u"]))) for s in snaps)
    print(f"{name}: {n} iterations, longest run {longest}, max|u| {worst:.3e}")
    assert np.all(np.isfinite(snaps[-1]["u"])) and worst <= 0.03, (name, worst)


def test_case_shapes():
    """What the cases are meant to exercise is there."""
    c1 = [a[1] for a in CC.case1(4)]
    assert c1 == [1, 11, 5, 2, 4] and sum(c1) == 23
    # two schedules back to back that end in one-step remainders, a call shorter than the depth, a schedule again
    assert c1[1] // 4 == 2 and c1[1] % 4 == 3 and c1[2] // 4 == 1 and c1[2] % 4 == 1 and c1[3] < 4 and c1[4] == 4
    c1b = [a[1] for a in CC.case1(5)[:4]]
    assert c1b == [1, 13, 6, 2] and sum(c1b) == 22
    assert [a[0] for a in CC.CASE2_WIDE] == ["step", "set_state", "step", "step"]
    assert [a[1] for a in CC.CASE2_WIDE if a[0] == "step"] == [1 + K + 2, 1 + 2 * K, 3]
    assert all(a[1] < 7 for a in CC.CASE2_REF if a[0] == "step")  # per-iteration kinematics at the default depth 7
    s, us, eps = CC.static_points(CC.WIDE)
    assert eps.size == 24 and s[0::2].min() > 280 and s[0::2].max() < 310 and s[1::2].max() < CC.NY - 2
    # REF: points at the periodic seam from iteration 0
    import oracle.oracle as O
    cil = O.Cilia(*CC.REF.cilia, CC.REF.nx)
    sx = cil.points(0)[0][0::2]
    assert sx.min() < 1.0 and sx.max() > CC.REF.nx - 1.0
    wx = O.Cilia(*CC.WIDE.cilia, CC.WIDE.nx).points(0)[0][0::2]
    assert wx.min() > 15 and wx.max() < 460


@pytest.mark.parametrize("name,cfg,actions", [("case1", CC.WIDE, CC.case1(4)), ("case6", CC.REF, CC.CASE6),
                                              ("case2 WIDE", CC.WIDE, CC.CASE2_WIDE), ("case2 REF", CC.REF, CC.CASE2_REF),
                                              ("group REF", CC.REF, CC.steps(*CC.GROUP_CALLS))])
@pytest.mark.parametrize("shift", [1])
def test_it_off_by_one_shows(oracle, name, cfg, actions, shift):
    """u_s(it = 0) is exactly 0, so an `it` one off moves the fields by O(1) relative, after every call."""
    _, good = CC.run_twin(oracle, cfg, actions)
    _, bad = CC.run_twin(oracle, cfg, actions, shift=shift)
    for i, (g, b) in enumerate(zip(good, bad)):
        d, m = moved(b, g)
        print(name, "shift", shift, "call", i, d)
        assert m >= POWER, (name, shift, i, d)


def test_zeroed_history_at_a_hand_over_shows_in_the_fields_only(oracle):
    """A fresh Cilia at the hand-over between the two schedules of case 1 (and, in a second run, between the
    second schedule and the short call): that iteration's u_s is lasts-free, about 230 lattice units per
    iteration, and the fields are wrong by orders of magnitude; the points and u_s at the end of the run are
    bit-identical again."""
    acts = CC.case1(4)
    calls = [a[1] for a in acts]
    _, good = CC.run_twin(oracle, CC.WIDE, acts)
    for k in (2, 3):
        at = sum(calls[:k])
        tw, bad = CC.run_twin(oracle, CC.WIDE, acts, fresh_at=[at])
        d, m = moved(bad[-1], good[-1])
        print("fresh Cilia at", at, d)
        assert m >= 1e5, (at, d)
        for key in ("s", "u_s", "eps"):
            assert np.array_equal(bad[-1][key], good[-1][key]), (at, key)
        # ... while the iteration of the hand-over itself had the lasts-free u_s
        one = CC.Twin(oracle, CC.WIDE, fresh_at=[at])
        one.step(at + 1)
        assert float(np.max(np.abs(one.cil.u_s))) > 100.0


@pytest.mark.parametrize("name,cfg,actions", [("WIDE", CC.WIDE, CC.CASE2_WIDE), ("REF", CC.REF, CC.CASE2_REF)])
def test_no_beat_restart_at_the_reset_shows(oracle, name, cfg, actions):
    _, good = CC.run_twin(oracle, cfg, actions)
    _, bad = CC.run_twin(oracle, cfg, actions, keep_beat=True)
    assert np.array_equal(good[0]["rho"], bad[0]["rho"])  # the same up to the reset
    for i in (1, 2):
        d, m = moved(bad[i], good[i])
        print(name, "no restart, call", i, d)
        assert m >= POWER, (name, i, d)
