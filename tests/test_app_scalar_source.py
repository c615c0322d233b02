"""The driver's IBLB_SCALAR_SOURCE=flux[,decay]: a uniform influx through the bottom wall and a bulk decay on the scalar
of IBLB_SCALAR.  Its <it>-scalar.dat rows equal a Lattice driven the same way within 1e-9 * (1 + |C|), the bound of
tests/test_gpu_scalar.py's driver test and for the same reason (cilia, a second process); without the variable the
files are those of a scalar without a source; without IBLB_SCALAR the variable is refused with status 2."""
import numpy as np
import pytest

import app_model as M
from test_app import ARGS, read, run_app

pytestmark = pytest.mark.gpu

TAU, STRIDE = 0.8, 7
FLUX, DECAY = 1e-3, 0.01


def assert_files_equal_a_lattice(gpu, tmp_path, source):
    """Every <it>-scalar.dat under tmp_path against a Lattice with the driver's cilia, seed and (if `source`) source;
    returns that lattice's final C and the seed."""
    p = M.params(ARGS)
    X, Y = p["XDIM"], M.YDIM
    c0 = np.zeros((Y, X))
    c0[: Y // 2] = 1.0
    lat = gpu.Lattice(X, Y, p["TAU"], p["TAU2"], max_points=M.LENGTH * p["c_num"])
    try:
        lat.set_state()
        lat.set_cilia(p["c_num"], float(p["c_space"]), p["T"], p["p_step"])
        lat.set_scalar(c0, tau=TAU, stride=STRIDE)
        if source:
            lat.set_scalar_source(decay=DECAY, wall_flux=(np.full(X, FLUX), None))
        done, files = 0, 0
        ii, jj = np.meshgrid(np.arange(X), np.arange(Y))
        for it in range(0, p["ITERATIONS"], p["INTERVAL"]):
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            rows = [ln.split("\t") for ln in read(tmp_path, M.paths(p)["raw"] + f"{it}-scalar.dat").split("\n") if ln]
            assert len(rows) == X * Y and all(len(g) == 3 for g in rows)
            col = lambda k, conv=float: np.array([conv(g[k]) for g in rows]).reshape(Y, X)
            assert np.array_equal(col(0, int), ii) and np.array_equal(col(1, int), jj)
            want = lat.scalar()
            assert lat.scalar_info()["updates"] == done // STRIDE
            err = np.abs(col(2) - want)
            print(f"it {it}: max |dC| {err.max():.3e}")
            assert np.all(err <= 1e-9 * (1.0 + np.abs(want))), it
            files += 1
        assert files > 1 and done > STRIDE
        return lat.scalar(), c0
    finally:
        lat.close()


def test_app_feeds_the_scalar(gpu, tmp_path):
    r = run_app(ARGS, tmp_path, IBLB_SCALAR=f"{TAU},{STRIDE}", IBLB_SCALAR_SOURCE=f"{FLUX},{DECAY}")
    assert r.returncode == 0, r.stdout + r.stderr
    c, c0 = assert_files_equal_a_lattice(gpu, tmp_path, source=True)
    # the source is in the files: the seed's sum is not kept
    assert abs(c.sum() - c0.sum()) > 1e-3 * c0.sum()


def test_app_without_the_variable_writes_the_scalar_as_before(gpu, tmp_path):
    r = run_app(ARGS, tmp_path, IBLB_SCALAR=f"{TAU},{STRIDE}")
    assert r.returncode == 0, r.stdout + r.stderr
    c, c0 = assert_files_equal_a_lattice(gpu, tmp_path, source=False)
    assert abs(c.sum() - c0.sum()) <= 1e-9 * c0.sum()  # between no-flux walls sum(C) is kept


@pytest.mark.parametrize("value", ["1e-3,0.01", "1e-3"])
def test_app_refuses_the_variable_without_a_scalar(gpu, tmp_path, value):
    r = run_app(ARGS, tmp_path, IBLB_SCALAR_SOURCE=value)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "IBLB_SCALAR_SOURCE" in r.stderr and "IBLB_SCALAR" in r.stderr


@pytest.mark.parametrize("value", ["abc", "1e-3,-0.01", "nan", "1e-3,inf", "1e-3,0.01,2", "1e-3,"])
def test_app_refuses_a_malformed_value(gpu, tmp_path, value):
    r = run_app(ARGS, tmp_path, IBLB_SCALAR=f"{TAU},{STRIDE}", IBLB_SCALAR_SOURCE=value)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "IBLB_SCALAR_SOURCE" in r.stderr
