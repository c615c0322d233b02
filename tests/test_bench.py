"""bench.py's plain run and its options: `--dump-outputs DIR` writes the state the timed steps end in
(the same from run to run, and the oracle's state after prime + warmup + steps iterations from the
seeded state), a plain run leaves out what `--full` adds, and a large lattice is dumped as a fixed sample."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY, STEPS, WARMUP = 256, 192, 14, 7  # two deep launches timed
PRIME = 252  # --prime-seconds 0.02: six cycles of 42 steps, a fixed count


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _run(args):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--nx", str(NX), "--ny", str(NY), "--prime-seconds", "0.02"] + args
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=REPO)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_state(gpu, oracle, tmp_path):
    from cuda_iblb_11_amd import workloads as W
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _run(["--dump-outputs", a])
    _run(["--dump-outputs", b])
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["dtype"] == "f64" and d["unit"] == "MLUPS"
    assert d["higher_is_better"] is True and d["value"] > 0 and d["prime"]["steps"] == PRIME
    # MLUPS = cells / time of one step (ms_per_step is rounded to 1e-5 ms, value to 0.01)
    assert abs(d["value"] - NX * NY / d["ms_per_step"] / 1e3) <= (1e-5 / d["ms_per_step"] + 1e-6) * d["value"] + 0.01
    assert d["cpu_baseline"] is None  # --full only
    assert d["state_finite"] is True
    assert sorted(os.listdir(a)) == ["rho.npy", "u.npy"]
    rho, u = np.load(os.path.join(a, "rho.npy")), np.load(os.path.join(a, "u.npy"))
    assert rho.dtype == np.float64 and u.dtype == np.float64 and rho.shape == (NX * NY,) and u.shape == (2, NX * NY)
    assert np.array_equal(rho, np.load(os.path.join(b, "rho.npy"))) and np.array_equal(u, np.load(os.path.join(b, "u.npy")))
    r0, u0 = W.perturbed_state(NX, NY, W.SEED)
    sim = oracle.Simulation(NX, NY, W.TAU, W.TAU2, rho=r0, u=u0, body_force=W.BODY_FORCE)
    sim.step(PRIME + WARMUP + STEPS)
    # the project's f64 bound (max |phi - phi_ref| / max |phi_ref| <= 1e-6)
    assert np.max(np.abs(rho - sim.rho)) <= 1e-6 * np.max(np.abs(sim.rho))
    assert np.max(np.abs(u.ravel() - sim.u)) <= 1e-6 * np.max(np.abs(sim.u))


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline(gpu):
    d = _run(["--full", "--cpu-seconds", "0.2"])
    assert d["state_finite"] is True
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["unit"] == "MLUPS"


def test_dump_samples_a_large_lattice(tmp_path):
    bench = _bench_module()
    n = 3 * bench.DUMP_CELLS + 17
    rho = np.arange(n, dtype=np.float64)
    u = np.stack([rho + 0.25, rho + 0.5])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rho, u.ravel(), 0, 1, 12345)
    r, v = np.load(tmp_path / "a" / "rho.npy"), np.load(tmp_path / "a" / "u.npy")
    assert r.shape == (bench.DUMP_CELLS,) and v.shape == (2, bench.DUMP_CELLS)
    assert r.nbytes + v.nbytes <= 64e6
    assert np.all(np.diff(r) > 0) and r[0] >= 0 and r[-1] < n  # distinct cells, one per stratum
    assert np.all(np.diff(r) < 2.0 * n / bench.DUMP_CELLS + 1)
    assert np.array_equal(v[0], r + 0.25) and np.array_equal(v[1], r + 0.5)  # rho and u of the same cells
    assert np.array_equal(r, np.load(tmp_path / "b" / "rho.npy")) and np.array_equal(v, np.load(tmp_path / "b" / "u.npy"))
    # a slab per rank: the budget is shared, the files are named by rank
    bench.dump_outputs(str(tmp_path / "c"), rho, u.ravel(), 1, 2, 12345)
    assert sorted(os.listdir(tmp_path / "c")) == ["rho_rank1.npy", "u_rank1.npy"]
    assert np.load(tmp_path / "c" / "rho_rank1.npy").shape == (bench.DUMP_CELLS // 2,)
