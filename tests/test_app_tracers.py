"""The driver's passive tracers: IBLB_TRACERS=nx_t,ny_t[,stride] makes `bin/IBLB` seed a regular grid of
tracers (x = (i + 0.5) XDIM / nx_t, y = (j + 0.5) (YDIM - 1) / ny_t, tracer i * ny_t + j), let the context
move them every `stride` iterations, and write <it>-tracers.dat beside the fluid files at every output
iteration: one line `x y laps` per tracer in lattice units, %.17g.

The rows are checked against Lattice.tracers of the same scenario stepped from Python in the driver's
own call pattern.  The scenario has cilia, and two runs differ by the arrival order of the IB spread's fp64
atomics, so the positions are compared at 1e-9 * (the tracer's path length + 1), the bound of
tests/test_gpu_tracers.py with IB points; before the first update they must be the seeds exactly.
"""
import os

import numpy as np
import pytest

import app_model as M
from test_app import ARGS, read, run_app

GRID = (4, 3, 2)


def grid_seeds(X, Y, nxt, nyt):
    x = np.array([(i + 0.5) * X / nxt for i in range(nxt) for j in range(nyt)])
    y = np.array([(j + 0.5) * (Y - 1) / nyt for i in range(nxt) for j in range(nyt)])
    return x, y


# ---- CPU: refused before any device is touched ------------------------------------------------------

def test_tracers_refused_under_a_launcher(tmp_path):
    p = run_app(ARGS, tmp_path, timeout=60, IBLB_TRACERS="4,3,2", WORLD_SIZE=2, RANK=0)
    assert p.returncode == 2 and "IBLB_TRACERS" in p.stderr and "one GPU" in p.stderr
    q = run_app(ARGS, tmp_path, timeout=60, IBLB_TRACERS="4,3,2", WORLD_SIZE=2, RANK=1)
    assert q.returncode == 2 and q.stderr == ""


def test_tracers_value_must_be_well_formed(tmp_path):
    for bad in ("4", "0,3", "4,0", "4,3,0", "4,-3", "x", "4,3,2,1", "4,3x", "4,3,2x", "4;3"):
        p = run_app(ARGS, tmp_path, timeout=60, IBLB_TRACERS=bad)
        assert p.returncode == 2 and "IBLB_TRACERS must be" in p.stderr, bad


# ---- GPU ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_app_writes_the_tracers(gpu, tmp_path):
    p = M.params(ARGS)
    X, Y = p["XDIM"], M.YDIM
    nxt, nyt, stride = GRID
    r = run_app(ARGS, tmp_path, IBLB_TRACERS=",".join(str(v) for v in GRID))
    assert r.returncode == 0, r.stdout + r.stderr

    x0, y0 = grid_seeds(X, Y, nxt, nyt)
    lat = gpu.Lattice(X, Y, p["TAU"], p["TAU2"], max_points=M.LENGTH * p["c_num"])
    try:
        lat.set_state()
        lat.set_cilia(p["c_num"], float(p["c_space"]), p["T"], p["p_step"])
        lat.set_tracers(x0, y0, stride=stride)
        done, updates = 0, 0
        px, py, pl = x0, y0, np.zeros(x0.size, dtype=np.int32)
        path = np.zeros(x0.size)
        for it in range(0, p["ITERATIONS"], p["INTERVAL"]):
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            x, y, laps = lat.tracers()
            path += np.abs(x - px + (laps - pl) * float(X)) + np.abs(y - py)
            px, py, pl = x, y, laps
            rows = [ln.split("\t") for ln in read(tmp_path, M.paths(p)["raw"] + f"{it}-tracers.dat").split("\n") if ln]
            assert len(rows) == nxt * nyt and all(len(g) == 3 for g in rows)
            gx = np.array([float(g[0]) for g in rows])
            gy = np.array([float(g[1]) for g in rows])
            gl = np.array([int(g[2]) for g in rows])
            assert lat.tracer_info()["updates"] == done // stride
            if done < stride:  # no update yet: the seeds, bit for bit (%.17g round-trips a double)
                assert np.array_equal(gx, x0) and np.array_equal(gy, y0) and not gl.any()
            bound = 1e-9 * (path + 1.0)
            print(f"it {it}: max |dx| {np.abs(gx - x).max():.3e} max |dy| {np.abs(gy - y).max():.3e}")
            assert np.array_equal(gl, laps)
            assert np.all(np.abs(gx - x) <= bound) and np.all(np.abs(gy - y) <= bound), it
        assert np.max(path) > 0  # the tracers moved
    finally:
        lat.close()


@pytest.mark.gpu
def test_app_without_the_variable_writes_no_tracer_file(gpu, tmp_path):
    p = M.params(ARGS)
    r = run_app(ARGS, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    names = os.listdir(str(tmp_path) + "/" + M.paths(p)["raw"])
    assert "0-fluid.dat" in names and not [n for n in names if n.endswith("-tracers.dat")], names
