"""The driver's windowed field output: IBLB_FIELDS_STRIDE=sx[,sy] makes `bin/IBLB` write
<it>-fields.dat beside every <it>-fluid.dat (x, y, u_x, u_y, vorticity in the fluid file's scales,
then the shear stress sxy in lattice units; a blank line after each window row).

The x, y, u_x, u_y columns must be the text of the same cells' entries in <it>-fluid.dat.  The
vorticity and stress columns are checked against Lattice.fields of the same scenario stepped from
Python in the driver's own call pattern, at relative 1e-5: the six printed digits (a %g number is
within 5e-6 of its value; two runs differ only by the arrival order of the IB spread's fp64 atomics,
parts in 1e16).
"""
import os

import numpy as np
import pytest

import app_model as M
from test_app import ARGS, read, run_app

STRIDE = (4, 2)


def rows(text):
    """Lines of a field file as lists of tokens, blank lines dropped, and the blank lines' count."""
    lines = text.split("\n")
    return [ln.split("\t") for ln in lines if ln], sum(1 for ln in lines[:-1] if not ln)


# ---- CPU: refused before any device is touched ------------------------------------------------------

def test_fields_stride_refused_under_a_launcher(tmp_path):
    p = run_app(ARGS, tmp_path, timeout=60, IBLB_FIELDS_STRIDE="4,2", WORLD_SIZE=2, RANK=0)
    assert p.returncode == 2 and "IBLB_FIELDS_STRIDE" in p.stderr and "one GPU" in p.stderr
    q = run_app(ARGS, tmp_path, timeout=60, IBLB_FIELDS_STRIDE="4,2", WORLD_SIZE=2, RANK=1)
    assert q.returncode == 2 and q.stderr == ""


def test_fields_stride_must_be_positive(tmp_path):
    for bad in ("0", "4,0", "x"):
        p = run_app(ARGS, tmp_path, timeout=60, IBLB_FIELDS_STRIDE=bad)
        assert p.returncode == 2 and "IBLB_FIELDS_STRIDE must be" in p.stderr, bad


# ---- GPU ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_app_writes_the_windowed_fields(gpu, tmp_path):
    p = M.params(ARGS)
    sx, sy = STRIDE
    X, Y = p["XDIM"], M.YDIM
    wnx, wny = (X - 1) // sx + 1, (Y - 1) // sy + 1
    r = run_app(ARGS, tmp_path, IBLB_FIELDS_STRIDE=f"{sx},{sy}")
    assert r.returncode == 0, r.stdout + r.stderr

    lat = gpu.Lattice(X, Y, p["TAU"], p["TAU2"], max_points=M.LENGTH * p["c_num"])
    try:
        lat.set_state()
        lat.set_cilia(p["c_num"], float(p["c_space"]), p["T"], p["p_step"])
        done = 0
        for it in range(0, p["ITERATIONS"], p["INTERVAL"]):
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            got, blanks = rows(read(tmp_path, M.paths(p)["raw"] + f"{it}-fields.dat"))
            fluid, _ = rows(read(tmp_path, M.paths(p)["raw"] + f"{it}-fluid.dat"))
            assert len(got) == wnx * wny and blanks == wny and len(fluid) == X * Y
            assert all(len(g) == 6 for g in got)
            ref = lat.fields(["vort", "sxy"], (0, 0, wnx, wny, sx, sy))
            vort = ref["vort"] * p["s_scale"] / p["x_scale"]
            for j in range(wny):
                for i in range(wnx):
                    g = got[j * wnx + i]
                    assert g[:4] == fluid[j * sy * X + i * sx][:4], (it, i, j)
                    for tok, exp in ((g[4], vort[j, i]), (g[5], ref["sxy"][j, i])):
                        assert abs(float(tok) - exp) <= 1e-5 * abs(exp), (it, i, j, tok, exp)
        # the last output is no trivial field
        assert np.max(np.abs(ref["vort"])) > 0 and np.max(np.abs(ref["sxy"])) > 0
    finally:
        lat.close()


@pytest.mark.gpu
def test_app_without_the_variable_writes_no_fields_file(gpu, tmp_path):
    p = M.params(ARGS)
    r = run_app(ARGS, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = str(tmp_path) + "/" + M.paths(p)["raw"]
    names = os.listdir(raw)
    assert "0-fluid.dat" in names and not [n for n in names if n.endswith("-fields.dat")], names
