"""Checkpoints that hold the observers (iblb_save_checkpoint_ex, iblb_load_checkpoint, iblb_checkpoint_info) on the
GPU: a run interrupted by a checkpoint against the uninterrupted run, every comparison `==` / np.array_equal.

The lattices have no Lagrangian points, a body force and a perturbed initial state: there the fluid restart is
bit-identical and the deep launches equal the one-step launches bit for bit, so an interrupted run and an
uninterrupted one agree in every bit however iblb_step cuts the calls.  (The cumulative flux Q is left out of the
comparisons: its per-wave partials are added with atomics, in an order that varies between runs of one binary;
tests/test_gpu_fused.py::test_checkpoint_restart.)

20 x 13 in f64 and f32: 13 rows leave rows of padding in every y-fastest plane of the device, so a file that leaked
the device's layout would not round-trip into the twin.  5 x 2: the two rows, and with them both walls, belong to one
lane.  (iblb_create refuses a lattice of one row, "need nx >= 1 and ny >= 2", so 5 x 2 is the smallest lattice in
which one lane holds both walls; with two rows there is one level to gauge, not two.)

The observers: a scalar of stride 3 with a _VALUE wall below and a _NOFLUX wall above, a source (a field, decay, the
wall-value array of the wall below), an uptake with a rate on the no-flux wall, the ends `value` with a profile and
`outflow`, gauges at two stations (one at XDIM-1) and two levels; 37 tracers of stride 5, some of them within one
update's displacement of x = 0 and x = XDIM; an average of stride 4 over a strided window, 3 bins, squares and ux*uy,
fields ux, uy, c, cux.  The save comes after 7 iterations, on no event's boundary; then 2 and 11 more."""
import os
import struct

import numpy as np
import pytest

import ckpt_format_ref as ref
from cuda_iblb_11_amd import _lib as L
from cuda_iblb_11_amd import workloads as W
from test_gpu_fields import BODY_FORCE
from test_gpu_scalar import seeded_c0

pytestmark = pytest.mark.gpu

CASES = [(20, 13, "f64"), (20, 13, "f32"), (5, 2, "f64")]
TAU_C = 0.8
PIECES = (7, 2, 11)


def window(nx, ny):
    return (1, 2, 6, 4, 3, 3) if ny == 13 else (0, 0, 3, 1, 2, 2)


def gauge_positions(nx, ny):
    return (nx // 2, nx - 1), ((0, ny - 2) if ny > 2 else (0,))


def tracer_seeds(nx, ny):
    """37 tracers: 8 a hair left of x = XDIM and 8 a hair right of x = 0 (whichever way the fluid moves there, one update
    carries some of them across), the rest spread over the lattice."""
    rng = np.random.default_rng(5)
    ye = np.linspace(0.2, ny - 1.2, 8) if ny > 2 else np.linspace(0.1, 0.9, 8)
    x = np.concatenate([np.full(8, nx - 1e-9), np.full(8, 1e-9), rng.uniform(0.5, nx - 0.5, 21)])
    y = np.concatenate([ye, ye, rng.uniform(0.0, ny - 1.0, 21)])
    return x, y


def new_lattice(gpu, nx, ny, precision, state=True, **kw):
    lat = gpu.Lattice(nx, ny, W.TAU, W.TAU2, precision=precision, body_force=BODY_FORCE, **kw)
    if state:
        lat.set_state(*W.perturbed_state(nx, ny, 7))
    return lat


def set_observers(lat, nx, ny, scalar_in_average=True):
    rng = np.random.default_rng(11)
    lat.set_scalar(seeded_c0(nx, ny), tau=TAU_C, stride=3, walls=((L.SCALAR_WALL_VALUE, 0.25), (L.SCALAR_WALL_NOFLUX, 0.0)))
    lat.set_scalar_source(source=1e-3 * rng.uniform(-1.0, 1.0, (ny, nx)), decay=1e-3,
                          wall_value=(0.25 + 0.01 * np.arange(nx), None))
    lat.set_scalar_uptake(rate=(None, 0.05 * (1.0 + np.arange(nx) / nx)))
    lat.set_scalar_ends(kind=("value", "outflow"), value=(0.3, 0.0), profile=(np.linspace(0.2, 0.4, ny), None))
    st, lv = gauge_positions(nx, ny)
    lat.set_scalar_gauges(stations=st, levels=lv)
    lat.set_tracers(*tracer_seeds(nx, ny), stride=5)
    names = ["ux", "uy", "c", "cux"] if scalar_in_average else ["ux", "uy"]
    lat.set_average(names, window(nx, ny), stride=4, nbins=3, squares=True, uxuy=True)


def set_other_observers(lat, nx, ny):
    """Observers that differ from set_observers' in every respect a load must overwrite."""
    lat.set_scalar(np.full((ny, nx), 0.5), tau=0.9, stride=2)
    lat.set_scalar_uptake(rate=(0.2 * np.ones(nx), 0.1 * np.ones(nx)))
    lat.set_scalar_gauges(stations=(0,))
    lat.set_tracers(np.linspace(0.5, nx - 0.5, 11), np.full(11, 0.5), stride=2)
    lat.set_average(["rho"], None, stride=3, nbins=2)


def snapshot(lat):
    """Everything a context answers about its state and its observers, but the flux: {name: value or array}."""
    s = {"steps": lat.steps, "f": lat.populations()}
    s["scalar_info"] = lat.scalar_info()
    s["source_info"] = lat.scalar_source_info()
    s["uptake_info"] = lat.scalar_uptake_info()
    s["ends_info"] = lat.scalar_ends_info()
    s["gauges_info"] = lat.scalar_gauges_info()
    if s["scalar_info"]["stride"]:
        s["g"] = lat.scalar_populations()
        s["c"] = lat.scalar()
        s["wall_flux"] = np.stack(lat.scalar_wall_flux())
    if s["source_info"]["present"]:
        s["source"] = lat.scalar_source()
    if s["uptake_info"]["present"]:
        up = lat.scalar_uptake()
        s["uptake"] = np.stack(up["total"] + up["last"])
        s["uptake_substeps"] = up["substeps"]
    if s["ends_info"]["present"]:
        e = lat.scalar_ends()
        s["ends"] = np.stack(e["total"] + e["last"])
        s["ends_substeps"] = e["substeps"]
    if s["gauges_info"]["stations"] or s["gauges_info"]["levels"]:
        g = lat.scalar_gauges()
        for k in ("right", "left", "up", "down"):
            s["gauge_" + k] = g[k]
        s["gauges_substeps"] = g["substeps"]
    s["tracer_info"] = lat.tracer_info()
    if s["tracer_info"]["n"]:
        s["tracer_x"], s["tracer_y"], s["tracer_laps"] = lat.tracers()
    s["average_info"] = lat.average_info()
    if s["average_info"]["fields"]:
        for b in range(s["average_info"]["nbins"]):
            a = lat.average(b)
            s["bin%d_samples" % b] = a["samples"]
            s["bin%d_sum" % b] = np.stack(list(a["sum"].values()))
            s["bin%d_sq" % b] = np.stack(list(a["sum_sq"].values())) if a["sum_sq"] else None
            s["bin%d_uxuy" % b] = a["sum_uxuy"]
    return s


def assert_same(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def with_all(s):
    return (s["scalar_info"]["stride"] == 3 and s["source_info"]["present"] and s["uptake_info"]["present"] and
            s["ends_info"]["present"] and s["gauges_info"]["stations"] and s["tracer_info"]["n"] == 37 and
            s["average_info"]["nbins"] == 3)


@pytest.mark.parametrize("nx,ny,precision", CASES)
def test_round_trip_into_a_fresh_context_and_over_other_observers(gpu, tmp_path, nx, ny, precision):
    ck = str(tmp_path / "all.ck")
    A, C = new_lattice(gpu, nx, ny, precision), new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision, state=False)  # created new, nothing set
    D = new_lattice(gpu, nx, ny, precision)               # holds other observers, and has run with them
    try:
        set_observers(A, nx, ny)
        set_observers(C, nx, ny)
        set_other_observers(D, nx, ny)
        D.step(5)
        A.step(PIECES[0])
        C.step(PIECES[0])
        A.save_checkpoint(ck, L.OBSERVERS)
        assert not os.path.exists(ck + ".tmp")
        assert gpu.checkpoint_info(ck) == {"step": 7, "observers": L.OBSERVERS}
        at_save = snapshot(A)
        assert with_all(at_save)
        # the schedules lie inside their strides at the save: the scalar has run twice, the tracers and the average once
        assert at_save["scalar_info"]["updates"] == 2 and at_save["tracer_info"]["updates"] == 1
        assert at_save["average_info"]["samples_total"] == 1
        assert np.any(at_save["tracer_laps"] != 0), "no tracer crossed x = 0 / XDIM before the save"
        assert at_save["uptake_substeps"] == at_save["ends_substeps"] == at_save["gauges_substeps"] == 6
        B.load_checkpoint(ck)
        D.load_checkpoint(ck)
        assert_same(snapshot(B), at_save, "fresh context, at the load")
        assert_same(snapshot(D), at_save, "over other observers, at the load")
        assert_same(snapshot(C), at_save, "the uninterrupted run, at the save")
        for n in PIECES[1:]:
            for lat in (A, B, C, D):
                lat.step(n)
            a = snapshot(A)
            assert_same(snapshot(B), a, "fresh context, after %d more" % n)
            assert_same(snapshot(D), a, "over other observers, after %d more" % n)
            assert_same(snapshot(C), a, "the uninterrupted run, after %d more" % n)
        # stride 3 set at iteration 0: events after 3, 6, 9, ..., 18 of the 20 iterations, whoever ran them
        assert a["steps"] == 20 and a["scalar_info"]["updates"] == 6 and a["tracer_info"]["updates"] == 4
        assert a["average_info"]["samples_total"] == 5 and [a["bin%d_samples" % b] for b in range(3)] == [2, 2, 1]
    finally:
        for lat in (A, B, C, D):
            lat.close()


def present_bits(s):
    return ((L.CKPT_SCALAR if s["scalar_info"]["stride"] else 0) | (L.CKPT_TRACERS if s["tracer_info"]["n"] else 0) |
            (L.CKPT_AVERAGE if s["average_info"]["fields"] else 0))


def test_each_subset_of_observers(gpu, tmp_path):
    """Only the requested and set observers come back, the others are removed; checkpoint_info reports the same bits;
    without a section the file is iblb_save_checkpoint's, byte for byte.  (The average here samples no scalar field, so
    that it can be saved without the scalar.)"""
    nx, ny, precision = 20, 13, "f64"
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision)
    try:
        set_observers(A, nx, ny, scalar_in_average=False)
        A.step(7)
        full = snapshot(A)
        plain = str(tmp_path / "plain.ck")
        A.save_checkpoint(plain)
        fluid = open(plain, "rb").read()
        for bits in range(8):
            ck = str(tmp_path / ("s%d.ck" % bits))
            A.save_checkpoint(ck, bits)
            data = open(ck, "rb").read()
            assert data[:len(fluid)] == fluid, bits
            assert (data == fluid) == (bits == 0), bits
            verdict, found = ref.scan(data, len(fluid))
            assert verdict == ref.OK and ref.observers(found) == bits, bits
            assert gpu.checkpoint_info(ck) == {"step": 7, "observers": bits}
            if bits % 2:  # over what the last load left, and over other observers
                set_other_observers(B, nx, ny)
            B.load_checkpoint(ck)
            got = snapshot(B)
            assert present_bits(got) == bits, bits
            want = {k: v for k, v in full.items()}
            blank = snapshot_of_nothing(B)
            keys = {L.CKPT_SCALAR: ("scalar_info", "source_info", "uptake_info", "ends_info", "gauges_info"),
                    L.CKPT_TRACERS: ("tracer_info",), L.CKPT_AVERAGE: ("average_info",)}
            for bit, infos in keys.items():
                if not bits & bit:
                    for k in infos:
                        want[k] = blank[k]
            want = {k: v for k, v in want.items() if k in got}
            assert_same(got, want, "subset %d" % bits)
        # a requested observer that is not set writes no section, and no error
        A.set_tracers([], [])
        ck = str(tmp_path / "no_tracers.ck")
        A.save_checkpoint(ck, L.OBSERVERS)
        assert gpu.checkpoint_info(ck)["observers"] == L.CKPT_SCALAR | L.CKPT_AVERAGE
        # nothing set: the bytes of iblb_save_checkpoint, whatever is asked for
        A.set_average([])
        A.remove_scalar()
        A.save_checkpoint(plain)
        A.save_checkpoint(ck, L.OBSERVERS)
        assert open(ck, "rb").read() == open(plain, "rb").read()
        assert gpu.checkpoint_info(ck) == {"step": 7, "observers": 0}
    finally:
        A.close()
        B.close()


_BLANK = {}


def snapshot_of_nothing(lat):
    """The *_info answers of a context without observers (taken once from a context that has none)."""
    if not _BLANK:
        import cuda_iblb_11_amd as P
        E = P.Lattice(lat.nx, lat.ny, W.TAU, W.TAU2, precision=lat.precision, body_force=BODY_FORCE)
        try:
            E.set_state(*W.perturbed_state(lat.nx, lat.ny, 7))
            _BLANK.update({k: v for k, v in snapshot(E).items() if k.endswith("_info")})
        finally:
            E.close()
    return _BLANK


def scalar_payload_offsets(nx, ny):
    """Offsets inside the scalar section's payload, from the layout above the checkpoint code of csrc/iblb_ctx.hip:
    8 int64 and 3 doubles, the populations, then the source, the uptake, the ends and the gauges."""
    at = {"stride": 2 * 8, "tau": 8 * 8}
    pos = 11 * 8 + 5 * nx * ny * 8
    pos += 8 + 8 + nx * ny * 8 + 4 * nx * 8    # source: present, decay, field, wall arrays
    pos += 2 * 8 + 6 * nx * 8                  # uptake: present, substeps, a / total / last
    at["end_kind"] = pos
    pos += 4 * 8 + 2 * 8 + 6 * ny * 8          # ends: kinds, present, substeps, values, value / total / last
    at["n_stations"] = pos
    at["station0"] = pos + 3 * 8
    return at


def test_refusals_leave_no_file_and_an_untouched_context(gpu, tmp_path):
    nx, ny, precision = 20, 13, "f64"
    A = new_lattice(gpu, nx, ny, precision)
    B = new_lattice(gpu, nx, ny, precision, state=False)
    try:
        set_observers(A, nx, ny)
        ck = str(tmp_path / "r.ck")

        def refused(code, bits):
            with pytest.raises(gpu.IblbError) as e:
                A.save_checkpoint(ck, bits)
            assert e.value.code == code, (bits, e.value)
            assert os.listdir(tmp_path) == [], bits

        refused(L.IBLB_ERR_STATE, L.OBSERVERS)  # before the first step
        A.step(7)
        refused(L.IBLB_ERR_ARG, 8)
        refused(L.IBLB_ERR_ARG, L.OBSERVERS | 64)
        refused(L.IBLB_ERR_ARG, L.CKPT_AVERAGE)  # the average samples c and cux
        refused(L.IBLB_ERR_ARG, L.CKPT_AVERAGE | L.CKPT_TRACERS)
        A.save_checkpoint(ck, L.OBSERVERS)
        good = open(ck, "rb").read()
        plain = str(tmp_path / "plain.ck")
        A.save_checkpoint(plain)
        fluid_end = os.path.getsize(plain)
        verdict, found = ref.scan(good, fluid_end)
        assert verdict == ref.OK and sorted(found) == [0, 1, 2, 3]
        sc, tr, av = (found[k][0] for k in (ref.SCALAR, ref.TRACERS, ref.AVERAGE))
        at = scalar_payload_offsets(nx, ny)
        assert struct.unpack_from("<q", good, sc + at["stride"])[0] == 3
        assert struct.unpack_from("<d", good, sc + at["tau"])[0] == TAU_C
        assert struct.unpack_from("<2q", good, sc + at["end_kind"]) == (L.SCALAR_END_VALUE, L.SCALAR_END_OUTFLOW)
        assert struct.unpack_from("<2q", good, sc + at["n_stations"]) == (2, 2)
        assert struct.unpack_from("<2q", good, sc + at["station0"]) == (nx // 2, nx - 1)

        def patched(offset, fmt, *values):
            b = bytearray(good)
            struct.pack_into(fmt, b, offset, *values)
            return bytes(b)

        bad = {
            "cut inside the scalar section": good[:sc + found[ref.SCALAR][1] // 2],
            "cut inside the tracer section": good[:tr + found[ref.TRACERS][1] // 2],
            "cut inside the average section": good[:av + found[ref.AVERAGE][1] // 2],
            "cut before the end section": good[:-16],
            "cut inside the end section": good[:-5],
            "a tag altered": patched(tr - 16, "<8s", b"IBLBTRX1"),
            "a length altered": patched(tr - 8, "<q", found[ref.TRACERS][1] + 8),
            "a length shortened by a section header": patched(sc - 8, "<q", found[ref.SCALAR][1] - 16),
            "the gauge count beyond XDIM": patched(sc + at["n_stations"], "<q", nx + 1),
            "a station beyond XDIM-1": patched(sc + at["station0"] + 8, "<q", nx),
            "stations not ascending": patched(sc + at["station0"], "<2q", nx - 1, nx // 2),
            "stride 0": patched(sc + at["stride"], "<q", 0),
            "tau 0.5": patched(sc + at["tau"], "<d", 0.5),
            "tau not finite": patched(sc + at["tau"], "<d", float("nan")),
            "a wall kind that does not exist": patched(sc + 3 * 8, "<q", 2),
            "an end kind that does not exist": patched(sc + at["end_kind"], "<q", 3),
            "another lattice in the scalar section": patched(sc, "<2q", ny, nx),
            "a tracer count that does not fit": patched(tr, "<q", 38),
            "a tracer outside the lattice": patched(tr + 4 * 8, "<d", float(nx)),
            "a window that leaves the lattice": patched(av + 2 * 8, "<q", 8),
            "an unknown field bit in the average": patched(av + 6 * 8, "<q", 1 << 20),
            "bin counts that do not add up": patched(av + 12 * 8, "<q", 5),
            "bytes behind the end section": good + b"\0" * 16,
            "an average of the scalar without a scalar section": good[:sc - 16] + good[tr - 16:],
        }
        before = snapshot(A)
        for name, data in bad.items():
            path = str(tmp_path / "bad.ck")
            with open(path, "wb") as f:
                f.write(data)
            with pytest.raises(gpu.IblbError) as e:
                A.load_checkpoint(path)
            assert e.value.code == L.IBLB_ERR_ARG, (name, e.value)
            assert_same(snapshot(A), before, name)
        # the framing's faults are checkpoint_info's too; the payloads' are not its business
        for name in ("cut inside the scalar section", "cut before the end section", "a tag altered", "a length altered",
                     "bytes behind the end section"):
            open(str(tmp_path / "bad.ck"), "wb").write(bad[name])
            with pytest.raises(gpu.IblbError) as e:
                gpu.checkpoint_info(str(tmp_path / "bad.ck"))
            assert e.value.code == L.IBLB_ERR_ARG, name
        # a twin that never tried: one further step agrees
        B.load_checkpoint(ck)
        A.step(4)
        B.step(4)
        assert_same(snapshot(A), snapshot(B), "one further step after the refused loads")
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_with_cilia_the_observers_return_as_saved(gpu, tmp_path, precision):
    """With the cilia on, the restart is bit-identical only up to the IB spread's summation order: the observers are
    compared at the moment of the load, and the run goes on from there."""
    nx, ny = 288, 192
    kw = dict(max_points=576)
    A = new_lattice(gpu, nx, ny, precision, **kw)
    B = new_lattice(gpu, nx, ny, precision, state=False, **kw)
    try:
        A.set_cilia(6, 48.0, 100000, 100000 // 6)
        set_observers(A, nx, ny)
        A.step(7)
        ck = str(tmp_path / "cilia.ck")
        A.save_checkpoint(ck, L.OBSERVERS)
        assert gpu.checkpoint_info(ck) == {"step": 7, "observers": L.OBSERVERS}
        a = {k: v for k, v in snapshot(A).items() if k != "f"}  # (the fluid: tests/test_gpu_fused.py)
        B.load_checkpoint(ck)  # the cilia configuration comes from the file
        b = {k: v for k, v in snapshot(B).items() if k != "f"}
        assert_same(b, a, "with cilia, at the load")
        B.step(7)
        after = snapshot(B)
        assert after["steps"] == 14 and after["scalar_info"]["updates"] == 4
        for k in ("f", "g", "c", "tracer_x", "tracer_y", "bin0_sum", "bin1_sum", "uptake", "ends", "gauge_right", "gauge_up"):
            assert np.all(np.isfinite(after[k])), k
    finally:
        A.close()
        B.close()


def test_a_group_slab_saves_no_section_and_refuses_a_file_with_sections(gpu, tmp_path, monkeypatch):
    """A context in an RCCL group (here one rank that is its own neighbour, IBLB_RCCL_SELF=1, as in
    tests/test_gpu_fused.py::test_rccl_self_ring) holds no observer: whatever is asked for, its file is
    iblb_save_checkpoint's; and a file with an observer part is refused with IBLB_ERR_UNSUPPORTED before anything is
    touched, while the same state without the observer part loads."""
    monkeypatch.setenv("IBLB_RCCL_SELF", "1")
    nx, ny, precision = 96, 200, "f64"
    A = new_lattice(gpu, nx, ny, precision)
    R = new_lattice(gpu, nx, ny, precision)
    try:
        set_observers(A, nx, ny)
        A.step(7)
        full, plain = str(tmp_path / "full.ck"), str(tmp_path / "plain.ck")
        A.save_checkpoint(full, L.OBSERVERS)
        A.save_checkpoint(plain)
        R.attach_rccl(gpu.rccl_unique_id(), 1, 0)
        R.step(3)
        mine, mine_ex = str(tmp_path / "mine.ck"), str(tmp_path / "mine_ex.ck")
        R.save_checkpoint(mine)
        R.save_checkpoint(mine_ex, L.OBSERVERS)
        assert open(mine_ex, "rb").read() == open(mine, "rb").read()
        before = snapshot(R)
        with pytest.raises(gpu.IblbError) as e:
            R.load_checkpoint(full)
        assert e.value.code == L.IBLB_ERR_UNSUPPORTED, e.value
        assert_same(snapshot(R), before, "after the refused load")
        R.load_checkpoint(plain)
        assert R.steps == 7 and np.array_equal(R.populations(), A.populations())
    finally:
        A.close()
        R.close()
