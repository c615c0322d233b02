"""Every reader of the C ABI on the slabs of a multi-rank RCCL group in the middle of a run: between deep
slab cycles (mode 0), per-iteration steps (0s, 1) and IB band cycles (2, 3).  There a reader does real
work (ctx_step.hip:prepare_read): a halo exchange of depth 1 or 3 on the context's stream and the owed IB
force of the slab's own columns, and it leaves the ghost and force state changed for the next iblb_step.

The cases run tests/mock_rccl/run_readers.py (ranks as threads on one GPU through the mock-RCCL build)
against a lone-slab twin; its docstring lists what is compared and where each bound comes from.  ROTATE
shifts which reader comes first at a read point: over the cases of a mode every reader is, at some read
point after a step, the call that meets the stale halo (test_every_reader_meets_the_stale_halo).

One more test reads the windowed readers on the real-RCCL self ring (IBLB_RCCL_SELF=1).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "mock_rccl"))
import run_readers as RUN  # noqa: E402
from test_gpu_reduce import blob  # noqa: E402

pytestmark = pytest.mark.gpu

# (mode, ranks, precision, depth, knobs, rotate)
CASES = [
    ("0", 2, "f64", 5, {}, 0), ("0", 3, "f64", 5, {}, 3), ("0", 4, "f32", 5, {}, 0), ("0", 3, "f32", 5, {}, 3),
    ("0", 3, "f64", 7, {}, 0),
    ("0", 2, "f64", 5, {"IBLB_OVERLAP": "0"}, 3),
    ("0", 3, "f64", 2, {}, 0),  # two-iteration sweeps, 2-column halo
    ("0s", 3, "f64", 5, {}, 0), ("0s", 2, "f32", 5, {}, 4),
    ("1", 2, "f64", 5, {}, 0), ("1", 4, "f64", 5, {}, 4), ("1", 3, "f32", 5, {}, 8),
    ("2", 2, "f64", 5, {}, 0), ("2", 3, "f32", 5, {}, 4),
    ("3", 2, "f64", 5, {}, 0), ("3", 4, "f32", 5, {}, 4),
    ("3", 3, "f64", 5, {"IBLB_BAND_PAR": "2"}, 0), ("3", 3, "f64", 5, {"IBLB_BAND_PAR": "0"}, 4),
    ("3", 2, "f64", 5, {"IBLB_BAND_MERGE": "0"}, 4),
]
KNOBS = ("IBLB_OVERLAP", "IBLB_SWEEP_DEPTH", "IBLB_BAND_PAR", "IBLB_BAND_MERGE")


def case_id(c):
    mode, n, precision, depth, knobs, _ = c
    return "-".join([f"mode{mode}", f"n{n}", precision, f"K{depth}"] + [f"{k[5:]}={v}" for k, v in knobs.items()])


def stale_first_readers(mode, depth, rotate):
    """The first collective reader of every read point after a step, as the runner orders them."""
    ib = mode in RUN.IB_MODES
    n_points = len(RUN.read_points(mode, depth)[1]) + 1
    return [RUN.first_reader(ib, p, p == n_points - 1, rotate) for p in range(1, n_points)]


def run(args, depth, knobs):
    # ranks as threads: 16 hardware queues keep the ranks' streams apart (test_rccl_slab_path_threads)
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs, IBLB_SWEEP_DEPTH=str(depth), GPU_MAX_HW_QUEUES="16")
    env.setdefault("IBLB_OVERLAP", "1")
    cmd = [sys.executable, os.path.join(HERE, "mock_rccl", "run_readers.py")] + [str(a) for a in args]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert lines, p.stdout + p.stderr[-3000:]
    print(lines[-1])
    res = json.loads(lines[-1])
    assert p.returncode == 0 and res["ok"], (res, p.stderr[-2000:])
    return res


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_readers_between_cycles(gpu, case):
    mode, n, precision, depth, knobs, rotate = case
    res = run([n, 48 * n, 130, mode, precision, rotate], depth, knobs)
    assert (res["mode"], res["n"], res["precision"], res["depth"]) == (mode, n, precision, depth), res
    # the readers that came first after a step are the ones the coverage test counts on
    want = stale_first_readers(mode, depth, rotate)
    assert res["first_reader_counts"] == {r: want.count(r) for r in set(want)}, res
    assert res["gather_ok"], res
    if mode in ("2", "3"):
        assert all(c >= 4 for c in res["band_cycles"]), res
    if mode == "0" and depth >= 3:
        assert all(c > 0 for c in res["sweepk_launches"]), res
        if knobs.get("IBLB_OVERLAP") != "0":  # (IBLB_OVERLAP=0: one stream, no device word to wait on)
            assert all(c > 0 for c in res["dev_wait_launches"]), res


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_count_nonfinite_on_a_group(gpu, precision):
    res = run([3, 144, 130, "0", precision, "nan"], 5, {})
    assert res["counts"] == [36, 36, 36] and res["rho_nonfinite"] == [0, 3, 1], res


def test_every_reader_meets_the_stale_halo():
    """Over the cases of each mode every reader comes first at some read point after a step."""
    for modes in (("0",), ("0s",), ("1",), ("2",), ("3",)):
        first = set()
        for mode, _, _, depth, _, rotate in CASES:
            if mode in modes:
                first.update(stale_first_readers(mode, depth, rotate))
        ib = modes[0] in RUN.IB_MODES
        every = {r for r in RUN.READERS if r != "window_local" and (ib or r != "lagrangian_force")}
        assert first == every, (modes, sorted(every - first))


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_self_ring_windowed_readers(gpu, monkeypatch, precision):
    """The real-RCCL self ring (one rank that is its own neighbour) against the lone slab, no IB, calls
    of 1, 7, 14 and 3 iterations at the default depth: populations, force, the local fields and their
    reduction are bit-equal after every call on the whole lattice and on a strided window."""
    from cuda_iblb_11_amd import workloads as W
    monkeypatch.setenv("IBLB_RCCL_SELF", "1")
    nx, ny = 96, 200
    rho, u = W.perturbed_state(nx, ny, 8)
    kw = dict(precision=precision, body_force=(1e-6, 2e-7))
    ref = gpu.Lattice(nx, ny, W.TAU, W.TAU2, **kw)
    ring = gpu.Lattice(nx, ny, W.TAU, W.TAU2, **kw)
    try:
        ref.set_state(rho, u)
        ring.set_state(rho, u)
        ring.attach_rccl(gpu.rccl_unique_id(), 1, 0)
        wins = [None, (1, 1, (nx - 2) // 3 + 1, (ny - 2) // 2 + 1, 3, 2)]
        for n in (1, 7, 14, 3):
            ref.step(n)
            ring.step(n)
            assert ring.window_local(None) == (0, nx)
            assert ring.count_nonfinite() == 0
            assert np.array_equal(ring.populations(), ref.populations()), n
            assert np.array_equal(ring.force(), ref.force()), n
            for w in wins:
                a, b = ring.fields(RUN.LOCAL, w), ref.fields(RUN.LOCAL, w)
                for m in RUN.LOCAL:
                    assert np.array_equal(a[m], b[m]), (n, w, m)
                assert blob(ring.reduce(RUN.REDUCED, w, rows=True, cols=True)) == \
                    blob(ref.reduce(RUN.REDUCED, w, rows=True, cols=True)), (n, w)
        assert ring.steps == ref.steps == 25
    finally:
        ref.close()
        ring.close()
