"""The driver's IBLB_SCALAR_STATIONS=x[,x...] and IBLB_SCALAR_LEVELS=y[,y...]: transport gauges for the scalar of
IBLB_SCALAR, and <it>-stations.dat and <it>-levels.dat beside <it>-scalar.dat with a pair of totals per gauge.  The
argument errors need no device: the driver refuses them with status 2 before it creates a context.  On the GPU the
columns equal Lattice.scalar_gauges() of a Lattice driven the same way within 1e-9 * (1 + |total|), the bound of
tests/test_gpu_scalar.py's driver test and for the same reason (cilia: the spread's atomic order differs between two
processes in the last bits of u); without the variables the driver writes what it wrote before and neither file."""
import os

import numpy as np
import pytest

import app_model as M
from test_app import ARGS, read, run_app

TAU, STRIDE = 0.8, 7
STATIONS, LEVELS = (0, 100, 287), (95, 96, 190)
NEW = ("-stations.dat", "-levels.dat")


def listed(v):
    return ",".join(str(n) for n in v)


# ---- argument errors: no device ------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [dict(IBLB_SCALAR_STATIONS="3"), dict(IBLB_SCALAR_LEVELS="4,9"),
                                 dict(IBLB_SCALAR_STATIONS="0,1", IBLB_SCALAR_LEVELS="2")])
def test_app_refuses_the_variables_without_a_scalar(tmp_path, env):
    r = run_app(ARGS, tmp_path, **env)
    assert r.returncode == 2, r.stdout + r.stderr
    assert sorted(env)[-1] in r.stderr and "needs IBLB_SCALAR" in r.stderr
    assert not any(f.endswith(NEW) for _, _, fs in os.walk(tmp_path) for f in fs)


@pytest.mark.parametrize("name", ["IBLB_SCALAR_STATIONS", "IBLB_SCALAR_LEVELS"])
@pytest.mark.parametrize("value", ["abc", "3,", ",3", "3,,4", "-1", "2.5", "1;2", "99999999999"])
def test_app_refuses_a_malformed_value(tmp_path, name, value):
    r = run_app(ARGS, tmp_path, IBLB_SCALAR=f"{TAU},{STRIDE}", **{name: value})
    assert r.returncode == 2, r.stdout + r.stderr
    assert name in r.stderr and "n[,n...]" in r.stderr


# ---- on the GPU ----------------------------------------------------------------------------------------------

def files_under(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.gpu
def test_app_writes_the_totals_of_a_lattice_twin(gpu, tmp_path):
    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    with_dir.mkdir()
    without_dir.mkdir()
    r = run_app(ARGS, with_dir, IBLB_SCALAR=f"{TAU},{STRIDE}", IBLB_SCALAR_STATIONS=listed(STATIONS),
                IBLB_SCALAR_LEVELS=listed(LEVELS))
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
        lat.set_scalar_gauges(stations=STATIONS, levels=LEVELS)
        done, files = 0, 0
        for it in range(0, p["ITERATIONS"], p["INTERVAL"]):
            lat.step(it + 1 - done)  # the driver writes after iteration `it`
            done = it + 1
            want = lat.scalar_gauges()
            assert want["substeps"] == (done // STRIDE) * STRIDE
            for name, n, length, pair in (("stations", len(STATIONS), Y, ("right", "left")),
                                          ("levels", len(LEVELS), X, ("up", "down"))):
                text = read(with_dir, M.paths(p)["raw"] + f"{it}-{name}.dat")
                rows = [ln.split("\t") for ln in text.split("\n") if ln]
                assert len(rows) == length and all(len(g) == 1 + 2 * n for g in rows), name
                assert [int(g[0]) for g in rows] == list(range(length)), name
                for k in range(n):
                    for j, key in enumerate(pair):
                        got = np.array([float(g[1 + 2 * k + j]) for g in rows])
                        err = np.abs(got - want[key][k])
                        print(f"it {it} {name} {k} {key}: sum {got.sum():.6e}, max |d total| {err.max():.3e}")
                        assert np.all(err <= 1e-9 * (1.0 + np.abs(want[key][k]))), (it, name, k, key)
            files += 1
        assert files > 1 and done > STRIDE
        # C = 1 below the middle and 0 above: the level under the step carried a net amount upwards
        k = LEVELS.index(Y // 2 - 1)
        assert np.all(want["up"][k] - want["down"][k] > 0.0) and np.all(want["right"][:, : Y // 2 - STRIDE - 1] > 0.0)
    finally:
        lat.close()
    # without the variables: neither file, every other file as with them
    r = run_app(ARGS, without_dir, IBLB_SCALAR=f"{TAU},{STRIDE}")
    assert r.returncode == 0, r.stdout + r.stderr
    plain = files_under(without_dir)
    assert plain and not any(f.endswith(NEW) for f in plain)
    assert plain == [f for f in files_under(with_dir) if not f.endswith(NEW)]
