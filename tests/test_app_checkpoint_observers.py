"""The driver's IBLB_CHECKPOINT / IBLB_RESTART with observers (the pattern of test_app.py's
test_app_restart_continues_the_run): the driver saves with IBLB_CKPT_OBSERVERS, and a restarted run goes on with the
scalar, its source, uptake, ends and gauges, the tracers and the averages the checkpoint held instead of seeding them
again.  One run of 20 iterations is uninterrupted; the other is the same run stopped at a checkpoint after 10
iterations and restarted.  The strides (3, 3, 4) do not divide 10.  The files both runs write at iteration 10 must be
byte-equal.  A restart from a checkpoint without an observer part, as an earlier driver wrote it, seeds the observers
as before."""
import os

import pytest

import app_model as M
import cuda_iblb_11_amd as P
from test_app import ARGS, read, run_app

pytestmark = pytest.mark.gpu

ENV = dict(IBLB_SCALAR="0.8,3,8,8", IBLB_SCALAR_SOURCE="1e-4,1e-3", IBLB_SCALAR_UPTAKE="0.05,0.02",
           IBLB_SCALAR_ENDS="value,outflow,0.3", IBLB_SCALAR_STATIONS="0,287", IBLB_SCALAR_LEVELS="95,190",
           IBLB_TRACERS="4,3,3", IBLB_AVERAGE="4,2,16,16", IBLB_STATS=1)
FILES = ("-scalar.dat", "-uptake.dat", "-ends.dat", "-stations.dat", "-levels.dat", "-tracers.dat", "-mean.dat")
FIRST = ARGS[:6] + ["0.0001", "1"] + ARGS[8:]  # ITERATIONS = 10, one output interval


def cstats_path(p):
    return M.paths(p)["flux"][:-len("-flux.dat")] + "-cstats.dat"


def test_app_restart_continues_the_observers(gpu, tmp_path):
    p = M.params(ARGS)
    assert M.params(FIRST)["ITERATIONS"] == 10 and p["ITERATIONS"] == 20 and p["INTERVAL"] == 10
    whole, cut = tmp_path / "whole", tmp_path / "cut"
    whole.mkdir()
    cut.mkdir()
    r = run_app(ARGS, whole, **ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    ck = str(tmp_path / "ck")
    r = run_app(FIRST, cut, IBLB_CHECKPOINT=ck, IBLB_CHECKPOINT_EVERY=10, **ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert P.checkpoint_info(ck + ".rank0") == {"step": 10, "observers": P.OBSERVERS}
    raw = M.paths(p)["raw"]
    assert not os.path.exists(str(cut) + "/" + raw + "10-scalar.dat")
    # the restart's environment asks for other observers (the output sampling aside, which no checkpoint holds): the
    # checkpoint's configuration wins
    other = dict(ENV, IBLB_SCALAR="0.9,5,8,8", IBLB_SCALAR_UPTAKE="0.5", IBLB_SCALAR_STATIONS="7", IBLB_TRACERS="2,2,1",
                 IBLB_AVERAGE="7,1,16,16")
    r = run_app(ARGS, cut, IBLB_RESTART=ck, **other)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in FILES:
        got, want = read(cut, raw + "10" + name), read(whole, raw + "10" + name)
        assert len(want) > 0, name
        assert got == want, name
    got, want = read(cut, cstats_path(p)).split("\n"), read(whole, cstats_path(p)).split("\n")
    assert len(got) == len(want) == 3 and want[1].startswith("10\t")
    assert got[1:] == want[1:]


def test_app_restart_without_an_observer_part_seeds_the_observers(gpu, tmp_path):
    """A checkpoint of a run without observers is the fluid part alone, as every earlier driver wrote it; the restart
    seeds what its environment names at the restart's first iteration, as it always has: one iteration later the
    scalar (stride 3) is still its seed, no total has moved, the tracers are where they were put, and the first output
    iteration writes no mean file."""
    p = M.params(ARGS)
    ck = str(tmp_path / "ck")
    r = run_app(FIRST, tmp_path, IBLB_CHECKPOINT=ck, IBLB_CHECKPOINT_EVERY=10)
    assert r.returncode == 0, r.stdout + r.stderr
    assert P.checkpoint_info(ck + ".rank0") == {"step": 10, "observers": 0}
    r = run_app(ARGS, tmp_path, IBLB_RESTART=ck, **ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = M.paths(p)["raw"]
    rows = [ln.split("\t") for ln in read(tmp_path, raw + "10-scalar.dat").split("\n") if ln]
    assert len(rows) == (287 // 8 + 1) * (191 // 8 + 1)
    # (C is the sum of five equilibrium populations, each rounded: within a few ulp of the seed's 1, exactly its 0)
    assert all(abs(float(c) - 1.0) <= 1e-14 if int(y) < M.YDIM // 2 else float(c) == 0.0 for _, y, c in rows)
    for name in ("-uptake.dat", "-ends.dat"):
        rows = [ln.split("\t") for ln in read(tmp_path, raw + "10" + name).split("\n") if ln]
        assert rows and all(float(a) == 0.0 and float(b) == 0.0 for _, a, b in rows), name
    rows = [ln.split("\t") for ln in read(tmp_path, raw + "10-tracers.dat").split("\n") if ln]
    assert [(float(x), float(y), int(n)) for x, y, n in rows] == \
        [((i + 0.5) * p["XDIM"] / 4, (j + 0.5) * (M.YDIM - 1) / 3, 0) for i in range(4) for j in range(3)]
    assert not os.path.exists(str(tmp_path) + "/" + raw + "10-mean.dat")
