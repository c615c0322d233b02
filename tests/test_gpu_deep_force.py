"""The deep sweep's collide for a body force along x only (iblb_device.h: relax_cells / relax_dev with XF;
lbm_sweep_impl.h: sweepk_kernel's XF builds of the f64 785 lone and slab kernels and of the f32 593 one).
The launcher takes it when the launch's force has F_y = +-0 and IBLB_DEEP_FORCE=general is not set, and it
must give every population the general collide gives, bit for bit.

The scheme is tests/test_gpu_deep_steady.py's: a deep run against the one-step path (IBLB_SWEEP=0) over calls
of 1 + 2K and 2K - 1 iterations on the row-parity state, the populations compared as integer bit patterns
(the float64 values the library returns, viewed as uint64: f32 storage is widened exactly) and the flux to
1e-13 relative (per-wave atomics: the order varies).  Every case runs twice, the default run
(deep_force_build() == 1) and IBLB_DEEP_FORCE=general (== 0): both must equal the one-step run.

* forces (1e-6, 0), (0, 0) and (-2e-6, -0); depths 3-7; the flux column at its default place and at 0;
* f64 on 40 x 300 (two inner chunks and the wall chunks) in balanced sweeps and in fixed sweeps of 16, and
  on 9 x 171 at depths 6 and 7 (one inner chunk, fewer columns than the walk's reach); f32 on 40 x 300;
* force (1e-6, 3e-7): the default run takes the general build (0);
* the RCCL self ring's 64 x 300 f64 slab (the ghost-column build, write-through walks in its edge waves)
  with force (1e-6, 0) against the lone slab after 1, 7 and 13 iterations: both took build 1.

The build of the last deep launch is MODE 785 / 593 at two cells per lane in both force builds; at depth 7,
where tests/test_gpu_fused.py:test_default_deep_builds pins them, (MODE, cells per lane, waves per SIMD,
VGPRs) is (785, 2, 1, 241) lone, (785, 2, 1, 243) slab and (593, 2, 3, 161) f32.  (The shallower kernels
have their own register counts and resident waves: depth 3 f64 has 193 VGPRs and two waves per SIMD.)

The reference of each (precision, shape, depth, force, flux column) is computed once and shared, read-only.
"""
import numpy as np
import pytest

import regimes as R
from test_gpu_deep_lockstep import DEEP_ENV, parity_state

pytestmark = pytest.mark.gpu

FORCES = [(1e-6, 0.0), (0.0, 0.0), (-2e-6, -0.0)]
FORCE_IDS = ["fx", "zero", "negfx_negzero"]
DEPTHS = [3, 4, 5, 6, 7]
FLUX_COLUMNS = [None, 0]
FLUX_IDS = ["qdefault", "q0"]
BUILD = {"f64": (785, 2, 1), "f32": (593, 2, 3)}
VGPRS7 = {"f64": 241, "f64slab": 243, "f32": 161}
_refs = {}


def _clean(monkeypatch):
    for name in DEEP_ENV + ("IBLB_RCCL_SELF", "IBLB_DEEP_FORCE"):
        monkeypatch.delenv(name, raising=False)


def _make(gpu, precision, nx, ny, force, flux_column=None):
    rho, u = parity_state(nx, ny)
    lat = gpu.Lattice(nx, ny, R.TAUS["Re1"][0], R.TAUS["Re1"][1], precision=precision, body_force=force,
                      flux_column=flux_column)
    lat.set_state(rho, u)
    lat.set_profiling(True)
    return lat


def _bits(f):
    return f.view(np.uint64)


def _one_step(gpu, monkeypatch, precision, nx, ny, depth, force, flux_column, calls):
    key = (precision, nx, ny, depth, FORCES.index(force) if force in FORCES else force, flux_column)
    if key not in _refs:
        _clean(monkeypatch)
        monkeypatch.setenv("IBLB_SWEEP", "0")
        ref = _make(gpu, precision, nx, ny, force, flux_column)
        assert ref.deep_force_build() == -1
        for n in calls:
            ref.step(n)
        tm = ref.timing()
        assert tm["sweepk_launches"] == 0 and tm["sweep_launches"] == 0, tm
        assert ref.deep_force_build() == -1  # (no deep launch)
        f = ref.populations()
        f.setflags(write=False)
        _refs[key] = (f, ref.flux)
        ref.close()
        monkeypatch.delenv("IBLB_SWEEP")
    return _refs[key]


def _check_build(lat, tm, precision, depth, slab=False):
    assert (tm["deep_mode"], tm["deep_vs"]) == BUILD[precision][:2], tm
    if depth == 7:
        got = (tm["deep_mode"], tm["deep_vs"], tm["deep_waves_per_simd"], tm["deep_vgprs"])
        assert got == BUILD[precision] + (VGPRS7[precision + ("slab" if slab else "")],), tm


def _deep_against_one_step(gpu, monkeypatch, precision, nx, ny, depth, force, flux_column, want_default=1, **env):
    calls = [1 + 2 * depth, 2 * depth - 1]
    f_ref, q_ref = _one_step(gpu, monkeypatch, precision, nx, ny, depth, force, flux_column, calls)
    assert q_ref != 0.0
    for word, want in ((None, want_default), ("general", 0)):
        _clean(monkeypatch)
        monkeypatch.setenv("IBLB_SWEEP_DEPTH", str(depth))
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        if word is not None:
            monkeypatch.setenv("IBLB_DEEP_FORCE", word)
        lat = _make(gpu, precision, nx, ny, force, flux_column)
        try:
            assert lat.deep_force_build() == -1
            for n in calls:
                lat.step(n)
            tm = lat.timing()
            f, q, build = lat.populations(), lat.flux, lat.deep_force_build()
        finally:
            lat.close()
        nbad = int(np.count_nonzero(_bits(f) != _bits(f_ref)))
        print("XFORCE", precision, nx, ny, "depth", depth, "force", force, "flux column", flux_column, env, "IBLB_DEEP_FORCE",
              word, "build", build, "mode", tm["deep_mode"], tm["deep_vs"], tm["deep_waves_per_simd"], tm["deep_vgprs"],
              "launches", tm["sweepk_launches"], "populations that differ", nbad, "dflux", abs(q - q_ref) / abs(q_ref))
        # depth 3 mixes no K - 1: its second call is one deep launch and one two-iteration sweep
        assert tm["sweepk_launches"] == (4 if depth >= 4 else 3) and tm["sweepk_depth"] == depth, tm
        assert build == want, (word, build)
        _check_build(lat, tm, precision, depth)
        assert nbad == 0, (word, nbad)
        assert abs(q - q_ref) <= 1e-13 * abs(q_ref), (word, q, q_ref)


@pytest.mark.parametrize("flux_column", FLUX_COLUMNS, ids=FLUX_IDS)
@pytest.mark.parametrize("balance", [1, 0], ids=["balanced", "fixed16"])
@pytest.mark.parametrize("force", FORCES, ids=FORCE_IDS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_f64_two_inner_chunks(gpu, monkeypatch, depth, force, balance, flux_column):
    _deep_against_one_step(gpu, monkeypatch, "f64", 40, 300, depth, force, flux_column, IBLB_DEEP_W=16,
                           IBLB_DEEP_BALANCE=balance)


@pytest.mark.parametrize("flux_column", FLUX_COLUMNS, ids=FLUX_IDS)
@pytest.mark.parametrize("force", FORCES, ids=FORCE_IDS)
@pytest.mark.parametrize("depth", [6, 7])
def test_f64_narrow(gpu, monkeypatch, depth, force, flux_column):
    """9 x 171: one inner chunk, one-column sweeps, columns the walk loads twice."""
    _deep_against_one_step(gpu, monkeypatch, "f64", 9, 171, depth, force, flux_column)


@pytest.mark.parametrize("flux_column", FLUX_COLUMNS, ids=FLUX_IDS)
@pytest.mark.parametrize("force", FORCES, ids=FORCE_IDS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_f32_packed(gpu, monkeypatch, depth, force, flux_column):
    _deep_against_one_step(gpu, monkeypatch, "f32", 40, 300, depth, force, flux_column)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_general_force_takes_the_general_build(gpu, monkeypatch, precision):
    """F_y != 0: build 0 with and without the environment word."""
    _deep_against_one_step(gpu, monkeypatch, precision, 40, 300, 7, (1e-6, 3e-7), None, want_default=0)


def test_environment_word_only(gpu, monkeypatch):
    """IBLB_DEEP_FORCE takes the word general: anything else makes iblb_create fail with IBLB_ERR_ARG."""
    for bad in ("", "1", "General", "general,"):
        monkeypatch.setenv("IBLB_DEEP_FORCE", bad)
        with pytest.raises(gpu.IblbError) as e:
            gpu.Lattice(16, 8, R.TAUS["Re1"][0], R.TAUS["Re1"][1])
        assert e.value.code == gpu.IBLB_ERR_ARG and "IBLB_DEEP_FORCE" in str(e.value), (bad, str(e.value))
    monkeypatch.setenv("IBLB_DEEP_FORCE", "general")
    gpu.Lattice(16, 8, R.TAUS["Re1"][0], R.TAUS["Re1"][1]).close()


def test_self_ring_slab(gpu, monkeypatch):
    """The self ring's slab with force (1e-6, 0): the interior sweep's edge waves walk write-through.  Equal to
    the lone slab bit for bit after 1, 7 and 13 iterations; both ran the x-only build."""
    _clean(monkeypatch)
    nx, ny, force = 64, 300, (1e-6, 0.0)
    ref = _make(gpu, "f64", nx, ny, force)
    monkeypatch.setenv("IBLB_RCCL_SELF", "1")
    ring = _make(gpu, "f64", nx, ny, force)
    try:
        ring.attach_rccl(gpu.rccl_unique_id(), 1, 0)
        for n in (1, 7, 13):
            ref.step(n)
            ring.step(n)
            f1, f2 = ref.populations(), ring.populations()
            nbad = int(np.count_nonzero(_bits(f1) != _bits(f2)))
            print("XFORCE ring after", n, "populations that differ", nbad, "builds", ref.deep_force_build(),
                  ring.deep_force_build())
            assert nbad == 0, (n, nbad)
        tm, tr = ring.timing(), ref.timing()
        assert tm["deep_launches"] == 3 and tm["deep_iterations"] == 20 and tm["sweepk_launches"] >= 3, tm
        assert ring.deep_force_build() == 1 and ref.deep_force_build() == 1
        _check_build(ring, tm, "f64", 7, slab=True)
        _check_build(ref, tr, "f64", 7)
        assert ref.flux != 0.0
        assert abs(ring.flux - ref.flux) <= 1e-13 * abs(ref.flux), (ring.flux, ref.flux)
    finally:
        ring.close()
        ref.close()
