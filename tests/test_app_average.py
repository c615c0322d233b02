"""The driver's averaged fields: IBLB_AVERAGE=stride[,nbins[,sx[,sy]]] makes `bin/IBLB` average rho, u_x, u_y,
their squares and u_x u_y on every sx-th column and sy-th row of the whole lattice (iblb_set_average) and, at
every output iteration after the run's first, write <it>-mean.dat beside the fluid files: one line
`bin x y n mean_rho mean_ux mean_uy var_ux var_uy cov_uxuy` per bin and sample in lattice units, %.17g, a blank
line after each window row; then it resets the sums.

The rows are checked against Lattice.average of the same scenario stepped from Python in the driver's own call
pattern.  bin, x, y and n must match exactly.  The scenario has cilia, and two runs differ by the arrival order
of the IB spread's fp64 atomics, so the means are compared at 1e-9 * (1 + |v|) (the project's f64 parity bound
for fields, tests/test_gpu_bulk.py) and the variances and covariances, differences of second moments, at
1e-9 * (1 + mean^2).
"""
import os

import numpy as np
import pytest

import app_model as M
from test_app import ARGS, read, run_app

AVERAGE = (2, 2, 4, 2)  # stride, nbins, sx, sy


# ---- CPU: refused before any device is touched ------------------------------------------------------

def test_average_refused_under_a_launcher(tmp_path):
    p = run_app(ARGS, tmp_path, timeout=60, IBLB_AVERAGE="2,2,4,2", WORLD_SIZE=2, RANK=0)
    assert p.returncode == 2 and "IBLB_AVERAGE" in p.stderr and "one GPU" in p.stderr
    q = run_app(ARGS, tmp_path, timeout=60, IBLB_AVERAGE="2,2,4,2", WORLD_SIZE=2, RANK=1)
    assert q.returncode == 2 and q.stderr == ""


def test_average_value_must_be_well_formed(tmp_path):
    for bad in ("0", "5,0", "5,2,0", "x", "5,2,1,1,1", "5;2", "5,2,1,0", "-5", "5,", ",5", "5,2x", " 5", "5.0"):
        p = run_app(ARGS, tmp_path, timeout=60, IBLB_AVERAGE=bad)
        assert p.returncode == 2 and p.stderr.startswith("IBLB_AVERAGE must be"), bad


# ---- GPU ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_app_writes_the_means(gpu, tmp_path):
    p = M.params(ARGS)
    X, Y = p["XDIM"], M.YDIM
    stride, nbins, sx, sy = AVERAGE
    r = run_app(ARGS, tmp_path, IBLB_AVERAGE=",".join(str(v) for v in AVERAGE))
    assert r.returncode == 0, r.stdout + r.stderr

    wnx, wny = (X - 1) // sx + 1, (Y - 1) // sy + 1
    lat = gpu.Lattice(X, Y, p["TAU"], p["TAU2"], max_points=M.LENGTH * p["c_num"])
    try:
        lat.set_state()
        lat.set_cilia(p["c_num"], float(p["c_space"]), p["T"], p["p_step"])
        lat.set_average(["rho", "ux", "uy"], window=(0, 0, wnx, wny, sx, sy), stride=stride, nbins=nbins,
                        squares=True, uxuy=True)
        raw = str(tmp_path) + "/" + M.paths(p)["raw"]
        done, files = 0, 0
        outputs = list(range(0, p["ITERATIONS"], p["INTERVAL"]))
        for it in outputs:
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            name = f"{it}-mean.dat"
            if it == outputs[0]:  # the run's first output iteration writes no mean file (and does not reset)
                assert not os.path.exists(raw + name)
                continue
            files += 1
            text = read(tmp_path, M.paths(p)["raw"] + name)
            blocks = text.split("\n\n")
            assert blocks[-1] == ""  # a blank line after every window row, the last included
            rows = [ln.split("\t") for ln in text.split("\n") if ln]
            assert all(len(g) == 10 for g in rows)
            at = 0
            for b in range(nbins):
                a = lat.average(b)
                n = a["samples"]
                if n == 0:
                    continue
                part = rows[at:at + wnx * wny]
                at += wnx * wny
                assert len(part) == wnx * wny
                col = lambda k, conv=float: np.array([conv(g[k]) for g in part]).reshape(wny, wnx)
                ii, jj = np.meshgrid(np.arange(wnx) * sx, np.arange(wny) * sy)
                assert np.all(col(0, int) == b) and np.all(col(3, int) == n)
                assert np.array_equal(col(1, int), ii) and np.array_equal(col(2, int), jj)
                mean = {k: a["sum"][k] / float(n) for k in ("rho", "ux", "uy")}
                for k, name_k in ((4, "rho"), (5, "ux"), (6, "uy")):
                    err = np.abs(col(k) - mean[name_k])
                    print(f"it {it} bin {b} mean {name_k}: max |d| {err.max():.3e}")
                    assert np.all(err <= 1e-9 * (1.0 + np.abs(mean[name_k]))), (it, b, name_k)
                var = {k: a["sum_sq"][k] / float(n) - mean[k] * mean[k] for k in ("ux", "uy")}
                cov = a["sum_uxuy"] / float(n) - mean["ux"] * mean["uy"]
                for k, ref, m2 in ((7, var["ux"], mean["ux"] ** 2), (8, var["uy"], mean["uy"] ** 2),
                                   (9, cov, np.abs(mean["ux"] * mean["uy"]))):
                    err = np.abs(col(k) - ref)
                    print(f"it {it} bin {b} column {k}: max |d| {err.max():.3e}")
                    assert np.all(err <= 1e-9 * (1.0 + m2)), (it, b, k)
            assert at == len(rows)
            # the expected counts: samples after iterations stride, 2 stride, ... since the set or the last reset
            assert sum(lat.average(b)["samples"] for b in range(nbins)) == lat.average_info()["samples_total"] > 0
            lat.reset_average()
        assert files > 0
    finally:
        lat.close()
