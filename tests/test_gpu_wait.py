"""The RCCL group's device-side waits against a late neighbour.

Inside a run of deep slab cycles the interior's edge waves wait on a device word that the comm
stream's boundary sweeps of the previous cycle set, and (two-way handshake, f32 default) the
boundary sweeps wait on a word the interior's edge waves count into; a group slab's band cycle lets
its boundary sweeps wait on a word the level-0 IB sets once the cycle's exchange has landed
(ctx_step.hip:deep_slab_step, ctx_band.hip:band_step, lbm_sweep_impl.h:edge_wait).  Every one of
those producers sits behind the cycle's RCCL exchange, i.e. behind the neighbour ranks' hosts.  A
rank that reaches its exchange late (the drop-in driver writing fluid.dat on rank 0, a checkpoint,
the caller's own work) must only delay the others, never fail them: the waits are bounded by
wall-clock time (600 s by default, iblb_set_wait_timeout), not by a poll count.

The late neighbour is played by IBLB_TEST_HOLD=<n>:<ms> on the REAL-RCCL self ring (one rank that
is its own left and right neighbour, IBLB_RCCL_SELF=1): exchange n since the attach starts behind a
one-wave kernel that a host thread releases ms milliseconds later, while the chained cycles behind
it are already in flight with their device waits armed.  Each case must stay equal to the lone slab
(bit for bit without IB, up to the spread atomics' order with IB) and must not report
IBLB_ERR_COMM; with the bound set below the hold the call must fail cleanly with IBLB_ERR_COMM, and
the context must run correctly again from a new state.
(Reference loop these cycles replace: main.cu:817-934.)
"""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = int(os.environ.get("IBLB_SWEEP_DEPTH", "7"))
HOLD_MS = 3000


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / (m if m > 0 else 1.0))


def _env(monkeypatch, hold=None, **env):
    monkeypatch.setenv("IBLB_RCCL_SELF", "1")
    monkeypatch.delenv("IBLB_RESERVE_CUS", raising=False)  # the device waits need reserved CUs (auto: 32)
    monkeypatch.delenv("IBLB_WAIT_TIMEOUT_S", raising=False)
    if hold is None:
        monkeypatch.delenv("IBLB_TEST_HOLD", raising=False)
    else:
        monkeypatch.setenv("IBLB_TEST_HOLD", f"{hold[0]}:{hold[1]}")
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _pair(gpu, nx, ny, precision, seed, max_points=0):
    from cuda_iblb_11_amd import workloads as W
    rho, u = W.perturbed_state(nx, ny, seed)
    kw = dict(precision=precision, body_force=(1e-6, 2e-7), max_points=max_points)
    ref = gpu.Lattice(nx, ny, W.TAU, W.TAU2, **kw)
    ring = gpu.Lattice(nx, ny, W.TAU, W.TAU2, **kw)
    ref.set_state(rho, u)
    ring.set_state(rho, u)
    ring.attach_rccl(gpu.rccl_unique_id(), 1, 0)
    ring.set_profiling(True)  # (mode 1: the done word is also checked against the host's count)
    return ref, ring, (rho, u)


def _slab_run(gpu, precision, chunks, nx=256, ny=512, seed=41, timeout=None):
    """Lone slab vs self ring in the given chunks; returns the ring, the seconds each ring call took
    and the state, after checking every chunk bit for bit."""
    ref, ring, st = _pair(gpu, nx, ny, precision, seed)
    if timeout is not None:
        ring.set_wait_timeout(timeout)
    secs = []
    for n in chunks:
        ref.step(n)
        t0 = time.perf_counter()
        ring.step(n)
        secs.append(time.perf_counter() - t0)
        r1, u1 = ref.macro()
        r2, u2 = ring.macro()
        assert np.array_equal(r1, r2) and np.array_equal(u1, u2), n
    return ref, ring, secs, st


# chunks: the boot iteration (one-step, exchange 0), then 10 chained deep cycles in one call
# (exchanges 1 .. 10), then a mixed call; the hold sits on exchange 4, mid-chain
SLAB_CHUNKS = (1, 10 * K, 2 * K - 1)


@pytest.mark.parametrize("precision,flag", [("f64", None), ("f32", None), ("f64", 1), ("f32", 2)])
def test_slab_chain_survives_late_exchange(gpu, monkeypatch, precision, flag):
    """A deep slab chain whose 4th exchange starts 3 s late: f64 runs the one-way hand-off by default
    (the interior's edge waves wait on the boundary sweeps' word), f32 the two-way one (the boundary
    sweeps also wait on the edge waves' done count); the other flavour of each too.  Equal to the lone
    slab bit for bit, no IBLB_ERR_COMM, and the held call really waited."""
    env = {} if flag is None else {"IBLB_EDGE_FLAG": flag}
    _env(monkeypatch, hold=(4, HOLD_MS), **env)
    ref, ring, secs, _ = _slab_run(gpu, precision, SLAB_CHUNKS)
    assert secs[1] >= 0.95 * HOLD_MS / 1e3, secs  # the exchange was held with the chain in flight
    tm = ring.timing()
    assert tm["dev_wait_launches"] >= 10, tm  # device waits armed in the held call
    assert ring.steps == ref.steps == sum(SLAB_CHUNKS)
    assert abs(ring.flux - ref.flux) <= 1e-13 * abs(ref.flux)
    ring.close()
    ref.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_slab_wait_timeout_fails_cleanly(gpu, monkeypatch, precision):
    """The same hold with the wait bound set to 0.5 s: the call fails with IBLB_ERR_COMM (it does not
    hang, crash or return wrong fields silently); after a new set_state the context steps correctly."""
    _env(monkeypatch, hold=(4, HOLD_MS))
    ref, ring, st = _pair(gpu, 256, 512, precision, 43)
    ring.set_wait_timeout(0.5)
    ref.step(1)
    ring.step(1)
    with pytest.raises(gpu.IblbError) as e:
        ring.step(10 * K)
    assert e.value.code == gpu.IBLB_ERR_COMM and "wait timeout" in str(e.value), str(e.value)
    # recovery: a new state (set_state waits for every stream, the hold included), a longer bound
    ring.set_wait_timeout(600.0)
    for lat in (ref, ring):
        lat.set_state(*st)
        lat.step(1)
        lat.step(3 * K)
    r1, u1 = ref.macro()
    r2, u2 = ring.macro()
    assert np.array_equal(r1, r2) and np.array_equal(u1, u2)
    ring.close()
    ref.close()


def _swaying(nx, n_fil=2, pts=40, period=30):
    def points(it):
        k = np.arange(pts)
        s_all, u_all = [], []
        for m in range(n_fil):
            ph = 2 * np.pi * (it + 7 * m) / period
            s = np.empty(2 * pts, np.float32)
            s[0::2] = (m + 0.5) * nx / n_fil + 0.37 + 2.0 * (k / pts) * np.sin(ph)
            s[1::2] = 2.0 + k
            us = np.zeros(2 * pts, np.float32)
            us[0::2] = 2.0 * (k / pts) * np.cos(ph) * 2 * np.pi / period * 0.05
            s_all.append(s)
            u_all.append(us)
        s = np.concatenate(s_all)
        return s, np.concatenate(u_all), np.ones(s.size // 2, np.int32)
    return points


def _schedule(points, t0, n):
    ent = [points(it) for it in range(t0, t0 + n)]
    return (np.stack([e[0] for e in ent]), np.stack([e[1] for e in ent]), np.stack([e[2] for e in ent]))


def _band_run(gpu, precision, chunks, timeout=None, nx=256, ny=128):
    pts = _swaying(nx)
    ref, ring, st = _pair(gpu, nx, ny, precision, 47, max_points=80)
    if timeout is not None:
        ring.set_wait_timeout(timeout)
    t, secs = 0, []
    for n in chunks:
        for lat in (ref, ring):
            lat.set_lagrangian_steps(*_schedule(pts, t, n))
            t0 = time.perf_counter()
            lat.step(n)
            if lat is ring:
                secs.append(time.perf_counter() - t0)
        t += n
        r1, u1 = ref.macro()
        r2, u2 = ring.macro()
        tol = 1e-12 if precision == "f64" else 1e-5
        assert rel(r2, r1) <= tol and rel(u2, u1) <= tol, n
    return ref, ring, secs


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_band_cycle_survives_late_exchange(gpu, monkeypatch, precision):
    """A group slab's IB band cycles (the last level beside the deep sweep, IBLB_BAND_PAR=2, whose
    boundary sweeps poll the word the level-0 IB sets behind the exchange) with the exchange of the
    3rd cycle of a 6-cycle call held 3 s: equal to the lone slab up to the spread atomics' order."""
    _env(monkeypatch, hold=(3, HOLD_MS), IBLB_BAND_PAR=2)
    ref, ring, secs = _band_run(gpu, precision, (1, 6 * K))
    assert secs[1] >= 0.95 * HOLD_MS / 1e3, secs
    tm = ring.timing()
    assert tm["band_par_cycles"] >= 6 and tm["dev_wait_launches"] >= 4, tm
    ring.close()
    ref.close()


def test_band_wait_timeout_fails_cleanly(gpu, monkeypatch):
    """The band cycle's hold with a 0.5 s bound: IBLB_ERR_COMM, not a hang or silent wrong fields."""
    _env(monkeypatch, hold=(3, HOLD_MS), IBLB_BAND_PAR=2)
    with pytest.raises(gpu.IblbError) as e:
        _band_run(gpu, "f64", (1, 6 * K), timeout=0.5)
    assert e.value.code == gpu.IBLB_ERR_COMM and "wait timeout" in str(e.value), str(e.value)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("flag", [0, 1, 2])
def test_edge_flag_modes(gpu, monkeypatch, precision, flag):
    """IBLB_EDGE_FLAG 0 (queue waits), 1 (two-way device hand-off), 2 (one way) in both precisions
    (only the per-precision defaults were run): bit-identical to the lone slab over a
    chained run with mixed depths and readers between calls; device waits armed unless 0; with
    profiling on, the two-way done word equals the host's edge-wave count at every call's end."""
    _env(monkeypatch, IBLB_EDGE_FLAG=flag)
    ref, ring, _, _ = _slab_run(gpu, precision, (1, 4 * K, 2 * K - 1, 5, 3 * K), seed=45)
    tm = ring.timing()
    assert (tm["dev_wait_launches"] > 0) == (flag != 0), tm
    ring.close()
    ref.close()


def test_slab_chain_default_handoff(gpu, monkeypatch):
    """The default environment (each precision's own hand-off, no knob set): a boot step, four chained
    deep cycles and a mixed call, bit-identical to the lone slab in both precisions."""
    _env(monkeypatch)
    for precision in ("f64", "f32"):
        ref, ring, _, _ = _slab_run(gpu, precision, (1, 4 * K, 2 * K - 1), seed=49)
        ring.close()
        ref.close()
