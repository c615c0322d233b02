"""The driver's history: IBLB_PROBES=nx_p,ny_p[,stride] makes `bin/IBLB` record u_x, u_y at a regular grid of probes
(x = (i + 0.5) XDIM / nx_p, y = (j + 0.5) (YDIM - 1) / ny_p, probe i * ny_p + j) every `stride` iterations and append
`it p x y ux uy` per record and probe to <..>-probes.dat beside the flux file; IBLB_PATHLINES=1 with IBLB_TRACERS
appends `it p x y laps` per record and tracer to <..>-paths.dat.  Lattice units, %.17g.

The rows are checked against Lattice.history of the same scenario stepped from Python in the driver's own call
pattern.  The scenario has cilia, and two runs differ by the arrival order of the IB spread's fp64 atomics, so values
are compared at 1e-9 * (|v| + 1) and positions at 1e-9 * (the tracer's path length + 1), the bounds of
tests/test_gpu_tracers.py and tests/test_app_tracers.py with IB points; iterations, probe numbers, probe positions
and laps must be equal.
"""
import os

import numpy as np
import pytest

import app_model as M
from test_app import ARGS, read, run_app
from test_app_tracers import grid_seeds

PROBES = (3, 4, 3)
TRACERS = (4, 3, 2)


def hist_file(p, kind):
    return M.paths(p)["flux"][:-len("-flux.dat")] + f"-{kind}.dat"


# ---- CPU: refused before any device is touched ------------------------------------------------------

def test_history_refused_under_a_launcher(tmp_path):
    p = run_app(ARGS, tmp_path, timeout=60, IBLB_PROBES="3,4,3", WORLD_SIZE=2, RANK=0)
    assert p.returncode == 2 and "IBLB_PROBES" in p.stderr and "one GPU" in p.stderr
    q = run_app(ARGS, tmp_path, timeout=60, IBLB_PROBES="3,4,3", WORLD_SIZE=2, RANK=1)
    assert q.returncode == 2 and q.stderr == ""


def test_probes_value_must_be_well_formed(tmp_path):
    for bad in ("4", "0,3", "4,0", "4,3,0", "4,-3", "x", "4,3,2,1", "4,3x", "4,3,2x", "4;3"):
        p = run_app(ARGS, tmp_path, timeout=60, IBLB_PROBES=bad)
        assert p.returncode == 2 and "IBLB_PROBES must be" in p.stderr, bad


def test_pathlines_need_tracers_and_one_history_only(tmp_path):
    p = run_app(ARGS, tmp_path, timeout=60, IBLB_PATHLINES=1)
    assert p.returncode == 2 and "IBLB_PATHLINES needs IBLB_TRACERS" in p.stderr
    q = run_app(ARGS, tmp_path, timeout=60, IBLB_PATHLINES=1, IBLB_TRACERS="4,3,2", IBLB_PROBES="3,4")
    assert q.returncode == 2 and "IBLB_PROBES and IBLB_PATHLINES" in q.stderr
    assert not os.path.exists(str(tmp_path) + "/" + hist_file(M.params(ARGS), "paths"))


# ---- GPU ---------------------------------------------------------------------------------------------

def model_run(gpu, p, setup):
    """The scenario stepped in the driver's call pattern; every record drained where the driver drains."""
    lat = gpu.Lattice(p["XDIM"], M.YDIM, p["TAU"], p["TAU2"], max_points=M.LENGTH * p["c_num"])
    try:
        lat.set_state()
        lat.set_cilia(p["c_num"], float(p["c_space"]), p["T"], p["p_step"])
        setup(lat)
        done, drained, parts = 0, 0, []
        stops = [it + 1 for it in range(0, p["ITERATIONS"], p["INTERVAL"])] + [p["ITERATIONS"]]
        for stop in stops:
            if stop > done:
                lat.step(stop - done)
                done = stop
            rec = lat.history_info()["recorded"]
            if rec > drained:
                parts.append(lat.history(drained, rec - drained))
                drained = rec
        return {k: np.concatenate([h[k] for h in parts]) for k in parts[0]}
    finally:
        lat.close()


def rows_of(tmp_path, p, kind, width):
    rows = [ln.split("\t") for ln in read(tmp_path, hist_file(p, kind)).split("\n") if ln]
    assert rows and all(len(g) == width for g in rows)
    return rows


@pytest.mark.gpu
def test_app_writes_the_probes(gpu, tmp_path):
    p = M.params(ARGS)
    nxp, nyp, stride = PROBES
    r = run_app(ARGS, tmp_path, IBLB_PROBES=",".join(str(v) for v in PROBES))
    assert r.returncode == 0, r.stdout + r.stderr
    x0, y0 = grid_seeds(p["XDIM"], M.YDIM, nxp, nyp)
    n = x0.size
    ref = model_run(gpu, p, lambda lat: lat.set_history(["ux", "uy"], x0, y0, stride=stride,
                                                        capacity=p["INTERVAL"] // stride + 1))
    nrec = p["ITERATIONS"] // stride
    assert ref["iteration"].tolist() == [stride * (m + 1) for m in range(nrec)]
    rows = rows_of(tmp_path, p, "probes", 6)
    assert len(rows) == nrec * n  # one line per record and probe
    col = lambda k, t=float: np.array([t(g[k]) for g in rows]).reshape(nrec, n)
    assert np.array_equal(col(0, int), np.repeat(ref["iteration"], n).reshape(nrec, n))
    assert np.array_equal(col(1, int), np.tile(np.arange(n), (nrec, 1)))
    assert np.array_equal(col(2), np.tile(x0, (nrec, 1))) and np.array_equal(col(3), np.tile(y0, (nrec, 1)))
    for k, m in ((4, "ux"), (5, "uy")):
        err = np.abs(col(k) - ref[m])
        print(f"{m}: max |d| {err.max():.3e}")
        assert np.all(err <= 1e-9 * (np.abs(ref[m]) + 1.0)), m
    assert np.max(np.abs(ref["ux"])) > 0 and not np.array_equal(ref["ux"][0], ref["ux"][-1])  # a series, and it moved


@pytest.mark.gpu
def test_app_writes_the_pathlines(gpu, tmp_path):
    p = M.params(ARGS)
    X = p["XDIM"]
    nxt, nyt, stride = TRACERS
    r = run_app(ARGS, tmp_path, IBLB_TRACERS=",".join(str(v) for v in TRACERS), IBLB_PATHLINES=1)
    assert r.returncode == 0, r.stdout + r.stderr
    x0, y0 = grid_seeds(X, M.YDIM, nxt, nyt)
    n = x0.size

    def setup(lat):
        lat.set_tracers(x0, y0, stride=stride)
        lat.set_history([], stride=stride, capacity=p["INTERVAL"] // stride + 1, follow_tracers=True)

    ref = model_run(gpu, p, setup)
    nrec = p["ITERATIONS"] // stride
    assert ref["iteration"].tolist() == [stride * (m + 1) for m in range(nrec)]
    rows = rows_of(tmp_path, p, "paths", 5)
    assert len(rows) == nrec * n  # one line per record and tracer
    col = lambda k, t=float: np.array([t(g[k]) for g in rows]).reshape(nrec, n)
    assert np.array_equal(col(0, int), np.repeat(ref["iteration"], n).reshape(nrec, n))
    assert np.array_equal(col(1, int), np.tile(np.arange(n), (nrec, 1)))
    assert np.array_equal(col(4, int), ref["laps"].astype(np.int64))
    # the path length up to each record, from the reference's own pathline
    px = np.vstack([x0[None, :], ref["x"]]) + X * np.vstack([np.zeros((1, n)), ref["laps"]])
    py = np.vstack([y0[None, :], ref["y"]])
    path = np.cumsum(np.abs(np.diff(px, axis=0)) + np.abs(np.diff(py, axis=0)), axis=0)
    bound = 1e-9 * (path + 1.0)
    ex, ey = np.abs(col(2) - ref["x"]), np.abs(col(3) - ref["y"])
    print(f"max |dx| {ex.max():.3e} max |dy| {ey.max():.3e}")
    assert np.all(ex <= bound) and np.all(ey <= bound)
    assert np.max(path) > 0  # the tracers moved
    names = os.listdir(str(tmp_path) + "/" + M.paths(p)["raw"])
    assert [m for m in names if m.endswith("-tracers.dat")]  # the tracer files are written as before


@pytest.mark.gpu
def test_app_without_the_variables_writes_no_history_file(gpu, tmp_path):
    p = M.params(ARGS)
    r = run_app(ARGS, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    flux_dir = os.path.dirname(str(tmp_path) + "/" + M.paths(p)["flux"])
    assert sorted(os.listdir(flux_dir)) == [os.path.basename(M.paths(p)["flux"])]
    names = os.listdir(str(tmp_path) + "/" + M.paths(p)["raw"])
    assert "0-fluid.dat" in names
    assert not [m for m in names if m.endswith(("-probes.dat", "-paths.dat"))], names
