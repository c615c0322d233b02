"""The driver's particles: IBLB_PARTICLES=D[,drift_y[,bottom[,top[,seed]]]] puts a motion model
(iblb_set_tracer_model) on the grid of IBLB_TRACERS and makes `bin/IBLB` write, at every output iteration,
<it>-fates.dat (`index status iteration x y` per tracer) and <it>-deposits.dat (`x bottom top` per column)
beside <it>-tracers.dat, which keeps its format.

The driver's scenario has cilia, and two runs differ by the arrival order of the IB spread's fp64 atomics: a
fate can flip on the last bit of a position.  So against Lattice stepped from Python in the driver's own call
pattern only the counts are compared; everything else is checked as an invariant of the files themselves.
"""
import os

import numpy as np
import pytest

import app_model as M
from test_app import ARGS, read, run_app
from test_app_tracers import grid_seeds

GRID = (12, 8, 2)
PARTICLES = "40,-0.05,absorb,absorb,11"
MODEL = dict(diffusivity=40.0, drift=(0.0, -0.05), walls=("absorb", "absorb"), seed=11)


# ---- CPU: refused before any device is touched ------------------------------------------------------

def test_particles_value_must_be_well_formed(tmp_path):
    for bad in ("x", "-1", "nan", "inf", "0.1,", "0.1,nan", "0.1,0,stick", "0.1,0,absorb,stick", "0.1,0,absorb,reflect,-1",
                "0.1,0,absorb,reflect,1.5", "0.1,0,absorb,reflect,1,2", "0.1;0", "0.1x", "0.1,0,absorb,reflect,99999999999999999999",
                ",0"):
        p = run_app(ARGS, tmp_path, timeout=60, IBLB_TRACERS="4,3,2", IBLB_PARTICLES=bad)
        assert p.returncode == 2 and "IBLB_PARTICLES must be" in p.stderr, bad


def test_particles_need_the_tracers(tmp_path):
    p = run_app(ARGS, tmp_path, timeout=60, IBLB_PARTICLES="0.1")
    assert p.returncode == 2 and "IBLB_PARTICLES" in p.stderr and "IBLB_TRACERS" in p.stderr
    assert not os.path.exists(str(tmp_path) + "/" + M.paths(M.params(ARGS))["raw"] + "0-fluid.dat")


def test_particles_refused_under_a_launcher(tmp_path):
    p = run_app(ARGS, tmp_path, timeout=60, IBLB_PARTICLES="0.1", WORLD_SIZE=2, RANK=0)
    assert p.returncode == 2 and "IBLB_PARTICLES" in p.stderr and "one GPU" in p.stderr
    q = run_app(ARGS, tmp_path, timeout=60, IBLB_PARTICLES="0.1", WORLD_SIZE=2, RANK=1)
    assert q.returncode == 2 and q.stderr == ""
    # with the tracers as well, the tracers are refused first
    p = run_app(ARGS, tmp_path, timeout=60, IBLB_TRACERS="4,3,2", IBLB_PARTICLES="0.1", WORLD_SIZE=2, RANK=0)
    assert p.returncode == 2 and "one GPU" in p.stderr


# ---- GPU ---------------------------------------------------------------------------------------------

def table(root, rel, kinds):
    rows = [ln.split("\t") for ln in read(root, rel).split("\n") if ln]
    assert all(len(r) == len(kinds) for r in rows), rel
    return [np.array([k(r[c]) for r in rows]) for c, k in enumerate(kinds)]


@pytest.mark.gpu
def test_app_writes_the_fates_and_the_deposits(gpu, tmp_path):
    p = M.params(ARGS)
    X, Y = p["XDIM"], M.YDIM
    nxt, nyt, stride = GRID
    n = nxt * nyt
    r = run_app(ARGS, tmp_path, IBLB_TRACERS=",".join(str(v) for v in GRID), IBLB_PARTICLES=PARTICLES)
    assert r.returncode == 0, r.stdout + r.stderr

    x0, y0 = grid_seeds(X, Y, nxt, nyt)
    lat = gpu.Lattice(X, Y, p["TAU"], p["TAU2"], max_points=M.LENGTH * p["c_num"])
    try:
        lat.set_state()
        lat.set_cilia(p["c_num"], float(p["c_space"]), p["T"], p["p_step"])
        lat.set_tracers(x0, y0, stride=stride)
        lat.set_tracer_model(**MODEL)
        done, prev = 0, None
        for it in range(0, p["ITERATIONS"], p["INTERVAL"]):
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            raw = M.paths(p)["raw"]
            idx, st, hit, x, y = table(tmp_path, raw + f"{it}-fates.dat", (int, int, int, float, float))
            col, bottom, top = table(tmp_path, raw + f"{it}-deposits.dat", (int, int, int))
            tx, ty, tl = table(tmp_path, raw + f"{it}-tracers.dat", (float, float, int))  # its format is kept
            assert np.array_equal(idx, np.arange(n)) and np.array_equal(col, np.arange(X))
            assert np.array_equal(tx, x) and np.array_equal(ty, y)
            assert np.all(np.isin(st, (0, 1, 2)))
            assert np.all((x >= 0) & (x < X) & (y >= 0) & (y <= Y - 1))
            assert np.all(y[st == 1] == 0.0) and np.all(y[st == 2] == Y - 1.0)
            assert np.all(hit[st == 0] == -1)
            assert np.all((hit[st != 0] % stride == 0) & (hit[st != 0] >= stride) & (hit[st != 0] <= done))
            for got, s in ((bottom, 1), (top, 2)):
                assert np.array_equal(got, np.bincount(np.floor(x[st == s]).astype(np.int64), minlength=X))
            if done < stride:  # no update yet: the seeds, all alive
                assert np.array_equal(x, x0) and np.array_equal(y, y0) and not st.any()
            if prev is not None:  # a deposited tracer never moves again
                was = prev[0] != 0
                for a, b in zip(prev, (st, hit, x, y)):
                    assert np.array_equal(a[was], b[was])
            prev = (st, hit, x, y)
            info = lat.tracer_model_info()
            print(f"it {it}: alive {np.sum(st == 0)} bottom {bottom.sum()} top {top.sum()}; Lattice: {info}")
            assert (info["alive"], info["at_bottom"], info["at_top"]) == (np.sum(st == 0), bottom.sum(), top.sum())
        # the case is not empty: tracers deposited at each wall and others are still alive
        assert bottom.sum() >= 3 and top.sum() >= 3 and np.sum(st == 0) >= 3
    finally:
        lat.close()


@pytest.mark.gpu
def test_app_without_the_variable_writes_neither_file(gpu, tmp_path):
    p = M.params(ARGS)
    r = run_app(ARGS, tmp_path, IBLB_TRACERS="4,3,2")
    assert r.returncode == 0, r.stdout + r.stderr
    names = os.listdir(str(tmp_path) + "/" + M.paths(p)["raw"])
    assert "0-tracers.dat" in names and not [n for n in names if n.endswith(("-fates.dat", "-deposits.dat"))], names
