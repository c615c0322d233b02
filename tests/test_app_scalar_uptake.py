"""The driver's IBLB_SCALAR_UPTAKE=k_bottom[,k_top]: uniform first-order uptake at the two no-flux walls of the scalar of
IBLB_SCALAR, and <it>-uptake.dat beside <it>-scalar.dat with the totals per column.  The argument errors need no
device: the driver refuses them with status 2 before it creates a context.  On the GPU the totals equal those of a
Lattice driven the same way within 1e-9 * (1 + |total|), the bound of tests/test_gpu_scalar.py's driver test and for
the same reason (cilia: the spread's atomic order differs between two processes in the last bits of u); without the
variable the driver writes what it wrote before and no uptake file."""
import os

import numpy as np
import pytest

import app_model as M
from test_app import ARGS, read, run_app

TAU, STRIDE = 0.8, 7
RATES = (0.1, 0.02)


# ---- argument errors: no device ------------------------------------------------------------------------------

@pytest.mark.parametrize("value", ["0.1,0.02", "0.1"])
def test_app_refuses_the_variable_without_a_scalar(tmp_path, value):
    r = run_app(ARGS, tmp_path, IBLB_SCALAR_UPTAKE=value)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "IBLB_SCALAR_UPTAKE" in r.stderr and "needs IBLB_SCALAR" in r.stderr
    assert not any(f.endswith("-uptake.dat") for _, _, fs in os.walk(tmp_path) for f in fs)


@pytest.mark.parametrize("value", ["abc", "-0.1", "0.1,-0.02", "nan", "0.1,inf", "0.1,0.02,0.3", "0.1,", ",0.1"])
def test_app_refuses_a_malformed_value(tmp_path, value):
    r = run_app(ARGS, tmp_path, IBLB_SCALAR=f"{TAU},{STRIDE}", IBLB_SCALAR_UPTAKE=value)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "IBLB_SCALAR_UPTAKE" in r.stderr and "k_bottom[,k_top]" in r.stderr


# ---- on the GPU ----------------------------------------------------------------------------------------------

def files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.gpu
def test_app_writes_the_totals_of_a_lattice_twin(gpu, tmp_path):
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    with_dir.mkdir()
    without_dir.mkdir()
    r = run_app(ARGS, with_dir, IBLB_SCALAR=f"{TAU},{STRIDE}", IBLB_SCALAR_UPTAKE=f"{RATES[0]},{RATES[1]}")
    assert r.returncode == 0, r.stdout + r.stderr
    p = M.params(ARGS)
    X, Y = p["XDIM"], M.YDIM
    c0 = np.zeros((Y, X))
    c0[: Y // 2] = 1.0
    lat = gpu.Lattice(X, Y, p["TAU"], p["TAU2"], max_points=M.LENGTH * p["c_num"])
    try:
        lat.set_state()
        lat.set_cilia(p["c_num"], float(p["c_space"]), p["T"], p["p_step"])
        lat.set_scalar(c0, tau=TAU, stride=STRIDE)
        lat.set_scalar_uptake(rate=(np.full(X, RATES[0]), np.full(X, RATES[1])))
        done, files = 0, 0
        for it in range(0, p["ITERATIONS"], p["INTERVAL"]):
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            text = read(with_dir, M.paths(p)["raw"] + f"{it}-uptake.dat")
            rows = [ln.split("\t") for ln in text.split("\n") if ln]
            assert len(rows) == X and all(len(g) == 3 for g in rows)
            assert [int(g[0]) for g in rows] == list(range(X))
            want = lat.scalar_uptake()
            assert want["substeps"] == (done // STRIDE) * STRIDE
            for k in range(2):
                got = np.array([float(g[1 + k]) for g in rows])
                err = np.abs(got - want["total"][k])
                print(f"it {it} wall {k}: sum {got.sum():.6e}, max |d total| {err.max():.3e}")
                assert np.all(err <= 1e-9 * (1.0 + np.abs(want["total"][k]))), (it, k)
            # the scalar's own file is still written, and holds the scalar under the uptake
            rows = [ln.split("\t") for ln in read(with_dir, M.paths(p)["raw"] + f"{it}-scalar.dat").split("\n") if ln]
            got = np.array([float(g[2]) for g in rows]).reshape(Y, X)
            assert np.all(np.abs(got - lat.scalar()) <= 1e-9 * (1.0 + np.abs(lat.scalar()))), it
            files += 1
        assert files > 1 and done > STRIDE
        total = lat.scalar_uptake()["total"]
        # the lower half starts at C = 1 beside the faster wall: it absorbed, and more than the far one
        assert np.all(total[0] < 0) and total[0].sum() < total[1].sum()
    finally:
        lat.close()
    # without the variable: no uptake file, every other file as with it
    r = run_app(ARGS, without_dir, IBLB_SCALAR=f"{TAU},{STRIDE}")
    assert r.returncode == 0, r.stdout + r.stderr
    plain = files_under(without_dir)
    assert plain and not any(f.endswith("-uptake.dat") for f in plain)
    assert plain == [f for f in files_under(with_dir) if not f.endswith("-uptake.dat")]
