"""The driver's IBLB_SCALAR_ENDS=left,right[,value_left[,value_right]]: open ends in x for the scalar of IBLB_SCALAR, and
<it>-ends.dat beside <it>-scalar.dat with the totals per row.  The argument errors need no device: the driver refuses
them with status 2 before it creates a context.  On the GPU the totals equal those of a Lattice driven the same way
within 1e-9 * (1 + |total|), the bound of tests/test_gpu_scalar.py's driver test and for the same reason (cilia: the
spread's atomic order differs between two processes in the last bits of u); without the variable the driver writes
what it wrote before and no ends file."""
import os

import numpy as np
import pytest

import app_model as M
from test_app import ARGS, read, run_app

TAU, STRIDE = 0.8, 7
ENDS = ("value", "outflow", 0.75)


# ---- argument errors: no device ------------------------------------------------------------------------------

@pytest.mark.parametrize("value", ["value,outflow", "noflux,noflux,0.5"])
def test_app_refuses_the_variable_without_a_scalar(tmp_path, value):
    r = run_app(ARGS, tmp_path, IBLB_SCALAR_ENDS=value)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "IBLB_SCALAR_ENDS" in r.stderr and "needs IBLB_SCALAR" in r.stderr
    assert not any(f.endswith("-ends.dat") for _, _, fs in os.walk(tmp_path) for f in fs)


@pytest.mark.parametrize("value", ["abc", "value", "value,outflow,nan", "value,sink", "value,outflow,1,0,3", "value,",
                                   ",outflow"])
def test_app_refuses_a_malformed_value(tmp_path, value):
    r = run_app(ARGS, tmp_path, IBLB_SCALAR=f"{TAU},{STRIDE}", IBLB_SCALAR_ENDS=value)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "IBLB_SCALAR_ENDS" in r.stderr and "left,right[,value_left[,value_right]]" in r.stderr


# ---- on the GPU ----------------------------------------------------------------------------------------------

def files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.gpu
def test_app_writes_the_totals_of_a_lattice_twin(gpu, tmp_path):
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    with_dir.mkdir()
    without_dir.mkdir()
    r = run_app(ARGS, with_dir, IBLB_SCALAR=f"{TAU},{STRIDE}", IBLB_SCALAR_ENDS=f"{ENDS[0]},{ENDS[1]},{ENDS[2]}")
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
        lat.set_scalar_ends(kind=ENDS[:2], value=(ENDS[2], 0.0))
        done, files = 0, 0
        for it in range(0, p["ITERATIONS"], p["INTERVAL"]):
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            text = read(with_dir, M.paths(p)["raw"] + f"{it}-ends.dat")
            rows = [ln.split("\t") for ln in text.split("\n") if ln]
            assert len(rows) == Y and all(len(g) == 3 for g in rows)
            assert [int(g[0]) for g in rows] == list(range(Y))
            want = lat.scalar_ends()
            assert want["substeps"] == (done // STRIDE) * STRIDE
            for k in range(2):
                got = np.array([float(g[1 + k]) for g in rows])
                err = np.abs(got - want["total"][k])
                print(f"it {it} end {k}: sum {got.sum():.6e}, max |d total| {err.max():.3e}")
                assert np.all(err <= 1e-9 * (1.0 + np.abs(want["total"][k]))), (it, k)
            # the scalar's own file is still written, and holds the scalar under the ends
            rows = [ln.split("\t") for ln in read(with_dir, M.paths(p)["raw"] + f"{it}-scalar.dat").split("\n") if ln]
            got = np.array([float(g[2]) for g in rows]).reshape(Y, X)
            assert np.all(np.abs(got - lat.scalar()) <= 1e-9 * (1.0 + np.abs(lat.scalar()))), it
            files += 1
        assert files > 1 and done > STRIDE
        total = lat.scalar_ends()["total"]
        # the upper half starts at C = 0 beside an inlet at 0.75: it gained there; the lower half at C = 1 lost
        assert total[0][Y // 2 + 1:].sum() > 0 and total[0][: Y // 2 - 1].sum() < 0
        assert np.any(total[1] != 0.0)
    finally:
        lat.close()
    # without the variable: no ends file, every other file as with it
    r = run_app(ARGS, without_dir, IBLB_SCALAR=f"{TAU},{STRIDE}")
    assert r.returncode == 0, r.stdout + r.stderr
    plain = files_under(without_dir)
    assert plain and not any(f.endswith("-ends.dat") for f in plain)
    assert plain == [f for f in files_under(with_dir) if not f.endswith("-ends.dat")]
