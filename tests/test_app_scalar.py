"""The driver's passive scalar on the CPU: IBLB_SCALAR=tau[,stride[,sx[,sy]]] is parsed and refused before any
device is touched: a malformed value exits with code 2, and under a launcher the knob is not available.  What
the driver writes with it is checked on the GPU (tests/test_gpu_scalar.py)."""
from test_app import ARGS, run_app


def test_scalar_refused_under_a_launcher(tmp_path):
    p = run_app(ARGS, tmp_path, timeout=60, IBLB_SCALAR="0.8,2,4,2", WORLD_SIZE=2, RANK=0)
    assert p.returncode == 2 and "IBLB_SCALAR is not available" in p.stderr and "one GPU" in p.stderr
    q = run_app(ARGS, tmp_path, timeout=60, IBLB_SCALAR="0.8,2,4,2", WORLD_SIZE=2, RANK=1)
    assert q.returncode == 2 and q.stderr == ""


def test_scalar_value_must_be_well_formed(tmp_path):
    for bad in ("0.5", "0.4,1", "0", "nan", "inf", "-0.8", "x", "0.8,0", "0.8,2,0", "0.8,2,1,0", "0.8,2,1,1,1", "0.8;2",
                "0.8,", ",0.8", "0.8,2x", " 0.8", "0.8,2.0", "0.8x", "0.8,-2", "1e999"):
        p = run_app(ARGS, tmp_path, timeout=60, IBLB_SCALAR=bad)
        assert p.returncode == 2 and p.stderr.startswith("IBLB_SCALAR must be"), bad
