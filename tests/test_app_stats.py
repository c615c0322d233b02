"""The driver's statistics file: IBLB_STATS=1 makes `bin/IBLB` append one line per output iteration to
<..>-stats.dat beside the flux file, from one iblb_reduce_fields call over the whole lattice:

  it  sum(rho)  sum(rho u_x)  sum(rho u_y)  sum(KE)  max(u^2)  x  y  Ma = sqrt(max u^2)/0.57735  non-finite rho

Every number is checked against Lattice.reduce of the same scenario stepped from Python in the
driver's own call pattern, at relative 1e-12: the numbers are printed with 17 significant digits, and
two runs differ only by the arrival order of the IB spread's fp64 atomics, parts in 1e16 (as
tests/test_app_fields.py notes).  The location of the maximum may differ between two runs at a
near-tie, so the printed location's u^2 is checked against the maximum instead.
"""
import math
import os

import pytest

import app_model as M
from test_app import ARGS, read, run_app

RTOL = 1e-12


def stats_path(p):
    return M.paths(p)["flux"].replace("-flux.dat", "-stats.dat")


# ---- CPU: refused before any device is touched ------------------------------------------------------

def test_stats_refused_under_a_launcher(tmp_path):
    p = run_app(ARGS, tmp_path, timeout=60, IBLB_STATS=1, WORLD_SIZE=2, RANK=0)
    assert p.returncode == 2 and "IBLB_STATS" in p.stderr and "one GPU" in p.stderr
    q = run_app(ARGS, tmp_path, timeout=60, IBLB_STATS=1, WORLD_SIZE=2, RANK=1)
    assert q.returncode == 2 and q.stderr == ""


# ---- GPU ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("bigdata", ["1", "0"])
def test_app_writes_the_statistics(gpu, tmp_path, bigdata):
    args = ARGS[:9] + [bigdata]
    p = M.params(args)
    X, Y = p["XDIM"], M.YDIM
    r = run_app(args, tmp_path, IBLB_STATS=1)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split("\t") for ln in read(tmp_path, stats_path(p)).split("\n") if ln]
    its = list(range(0, p["ITERATIONS"], p["INTERVAL"]))
    assert [int(ln[0]) for ln in lines] == its and all(len(ln) == 10 for ln in lines)

    lat = gpu.Lattice(X, Y, p["TAU"], p["TAU2"], max_points=M.LENGTH * p["c_num"])
    try:
        lat.set_state()
        lat.set_cilia(p["c_num"], float(p["c_space"]), p["T"], p["p_step"])
        done = 0
        for it, ln in zip(its, lines):
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            s = lat.reduce(["rho", "momx", "momy", "ke", "usq"])
            exp = [s["rho"].sum, s["momx"].sum, s["momy"].sum, s["ke"].sum, s["usq"].max]
            for k, e in enumerate(exp):
                print(f"it {it} column {k + 1}: driver {ln[k + 1]} python {e!r}")
                assert abs(float(ln[k + 1]) - e) <= RTOL * abs(e), (it, k, ln[k + 1], e)
            x, y = int(ln[6]), int(ln[7])
            assert 0 <= x < X and 0 <= y < Y
            at = lat.reduce("usq", (x, y, 1, 1, 1, 1))["usq"].max
            assert abs(at - s["usq"].max) <= RTOL * s["usq"].max, (it, x, y, at, s["usq"].max)
            ma = math.sqrt(s["usq"].max) / 0.57735
            assert abs(float(ln[8]) - ma) <= RTOL * ma and int(ln[9]) == s["rho"].nonfinite == 0
        assert s["usq"].max > 0 and s["ke"].sum > 0  # the last output is no trivial state
    finally:
        lat.close()


@pytest.mark.gpu
def test_app_without_the_variable_writes_no_statistics(gpu, tmp_path):
    p = M.params(ARGS)
    r = run_app(ARGS, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    names = os.listdir(str(tmp_path) + "/Flux")
    assert [n for n in names if n.endswith("-flux.dat")] and not [n for n in names if n.endswith("-stats.dat")], names
