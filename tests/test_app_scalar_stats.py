"""The driver's scalar statistics: IBLB_SCALAR with IBLB_STATS=1 makes `bin/IBLB` append one line per output
iteration to <..>-cstats.dat beside the flux file, from one iblb_reduce_fields call over the whole lattice:

  it  sum(C)  sum(C^2)  min C  max C  sum(C u_x)  sum(C u_y)

Every number is checked against Lattice.reduce(["c", "cux", "cuy"]) of the same scenario stepped from Python in the
driver's own call pattern, at the relative 1e-12 of tests/test_app_stats.py (the driver is a second process with
cilia: two runs differ by the arrival order of the IB spread's fp64 atomics).  -stats.dat keeps its ten columns.
"""
import os

import numpy as np
import pytest

import app_model as M
from test_app import ARGS, read, run_app
from test_app_stats import RTOL, stats_path

pytestmark = pytest.mark.gpu

SCALAR = (0.8, 7)  # tau, stride


def cstats_path(p):
    return M.paths(p)["flux"].replace("-flux.dat", "-cstats.dat")


def test_app_writes_the_scalar_statistics(gpu, tmp_path):
    p = M.params(ARGS)
    X, Y = p["XDIM"], M.YDIM
    tau, stride = SCALAR
    r = run_app(ARGS, tmp_path, IBLB_STATS=1, IBLB_SCALAR=",".join(str(v) for v in SCALAR))
    assert r.returncode == 0, r.stdout + r.stderr
    its = list(range(0, p["ITERATIONS"], p["INTERVAL"]))
    lines = [ln.split("\t") for ln in read(tmp_path, cstats_path(p)).split("\n") if ln]
    assert [int(ln[0]) for ln in lines] == its and all(len(ln) == 7 for ln in lines)
    old = [ln.split("\t") for ln in read(tmp_path, stats_path(p)).split("\n") if ln]
    assert [int(ln[0]) for ln in old] == its and all(len(ln) == 10 for ln in old)

    c0 = np.zeros((Y, X))
    c0[: Y // 2] = 1.0
    lat = gpu.Lattice(X, Y, p["TAU"], p["TAU2"], max_points=M.LENGTH * p["c_num"])
    try:
        lat.set_state()
        lat.set_cilia(p["c_num"], float(p["c_space"]), p["T"], p["p_step"])
        lat.set_scalar(c0, tau=tau, stride=stride)
        done = 0
        for it, ln in zip(its, lines):
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            s = lat.reduce(["c", "cux", "cuy"])
            exp = [s["c"].sum, s["c"].sum_sq, s["c"].min, s["c"].max, s["cux"].sum, s["cuy"].sum]
            for k, e in enumerate(exp):
                print(f"it {it} column {k + 1}: driver {ln[k + 1]} python {e!r}")
                assert abs(float(ln[k + 1]) - e) <= RTOL * abs(e), (it, k, ln[k + 1], e)
            assert s["c"].nonfinite == 0 and s["c"].count == X * Y
        assert lat.scalar_info()["updates"] == done // stride > 0
        assert s["c"].min < 0.5 < s["c"].max and s["c"].sum_sq < s["c"].sum  # the step has diffused
    finally:
        lat.close()


def test_app_without_stats_writes_no_scalar_statistics(gpu, tmp_path):
    p = M.params(ARGS)
    r = run_app(ARGS, tmp_path, IBLB_SCALAR=",".join(str(v) for v in SCALAR))
    assert r.returncode == 0, r.stdout + r.stderr
    names = os.listdir(str(tmp_path) + "/Flux")
    assert [n for n in names if n.endswith("-flux.dat")] and not [n for n in names if n.endswith("stats.dat")], names
    r = run_app(ARGS, tmp_path, IBLB_STATS=1)
    assert r.returncode == 0, r.stdout + r.stderr
    names = os.listdir(str(tmp_path) + "/Flux")
    assert [n for n in names if n.endswith("-stats.dat")] and not [n for n in names if n.endswith("-cstats.dat")], names
