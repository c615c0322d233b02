"""The deep sweep's launch planner (csrc/deep_plan.h) on the CPU: tests/deep_plan_main.cpp, built with
AddressSanitizer + UndefinedBehaviorSanitizer (oracle/Makefile.san), run as a child process and checked
against tests/deep_plan_ref.py (an independent restatement from DESIGN §4), against known answers from
the project's record, and against brute-force enumeration of the sweeps.  Any sanitizer finding aborts
the program (-fno-sanitize-recover).

The edge-wave count is what a slab's interior waits for on the device, so a wrong one is a hang, not a
failed assert: it is checked here against a count over the enumerated sweeps' columns."""
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import deep_plan_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(REPO, "oracle", "_san", "deep_plan_san")
INT_MAX = 2**31 - 1
DEPTHS = (3, 4, 5, 6, 7)
FEATURES = list(itertools.product((0, 1), repeat=3))  # (split, pack, window)


@pytest.fixture(scope="module")
def planner():
    r = subprocess.run(["make", "-s", "-f", os.path.join(REPO, "oracle", "Makefile.san"), SAN], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([SAN], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600, env=e)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        out = [json.loads(ln) for ln in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def choose_line(f32, vs, slab, K, nskip, feat, ny_lo, ny_hi=None):
    return "choose %d %d %d %d %d %d %d %d %d %d" % (f32, vs, slab, K, nskip, *feat, ny_lo, ny_lo if ny_hi is None else ny_hi)


def choose_one(planner, f32, vs, slab, K, ny, nskip, feat):
    (o,) = planner([choose_line(f32, vs, slab, K, nskip, feat, ny)])
    return dict(zip(("mode", "wpe", "nch", "wall_top", "wall_ch0"), o["c"][0]))


# ---- known answers ----
DEFAULT_F64, DEFAULT_F32 = (1, 0, 1), (1, 1, 1)  # the context's default features
SPLIT_ONLY, PLAIN = (1, 0, 0), (0, 0, 0)         # what the band cycle asks for


@pytest.mark.parametrize("f32, vs, slab, ny, nskip, feat, want", [
    (0, 2, 0, 300, 0, DEFAULT_F64, (785, 1)),  # f64 lone
    (0, 2, 0, 63, 0, DEFAULT_F64, (1, 1)),
    (1, 2, 0, 300, 0, DEFAULT_F32, (593, 3)),  # f32 lone
    (1, 2, 0, 63, 0, DEFAULT_F32, (65, 1)),
    (0, 2, 1, 512, 0, DEFAULT_F64, (785, 1)),  # slabs
    (1, 1, 1, 512, 0, DEFAULT_F32, (273, 4)),
    (0, 2, 0, 160, 0, SPLIT_ONLY, (273, 1)),   # the band cycle's deep sweeps
    (0, 2, 0, 160, 3, SPLIT_ONLY, (129, 1)),
    (1, 2, 0, 160, 0, PLAIN, (1, 1)),
    (1, 1, 0, 300, 3, SPLIT_ONLY, (401, 3)),   # f32, one cell per lane, lone: the split with skip regions
])
def test_known_builds_depth7(planner, f32, vs, slab, ny, nskip, feat, want):
    c = choose_one(planner, f32, vs, slab, 7, ny, nskip, feat)
    assert (c["mode"], c["wpe"]) == want


def test_known_split_rows(planner):
    """f64, two cells per lane, 300 rows at depth 7: rows [0, 52) | two inner chunks | [248, 300)."""
    c = choose_one(planner, 0, 2, 0, 7, 300, 0, DEFAULT_F64)
    assert (c["wall_top"], c["wall_ch0"]) == (248, 2)


@pytest.mark.parametrize("split, W, slots, want", [
    (1, 128, 1024, dict(nsweep=27, nsweep_w=27, waves=999, rounds=1)),   # f64 (785 build, one wave per SIMD)
    (1, 96, 1024, dict(nsweep=55, nsweep_w=55, waves=2035, rounds=2)),   # f64 at the narrower sweeps: two rounds
    (1, 128, 3072, dict(nsweep=83, nsweep_w=83, waves=3071)),            # f32 (593 build, three waves per SIMD)
])
def test_known_sweeps_4096(planner, split, W, slots, want):
    """4096 x 4096 at depth 7, two cells per lane: 35 inner chunks."""
    c = choose_one(planner, 0, 2, 0, 7, 4096, 0, DEFAULT_F64)
    assert c["wall_ch0"] == 35
    (o,) = planner(["sweeps %d 2 0 4096 0 %d 32 %d 35 %d 0 0" % (split, W, c["nch"], slots)])
    assert {k: o[k] for k in want} == want


# ---- the choice, exhaustively ----
@pytest.mark.parametrize("K", DEPTHS)
def test_choice_exhaustive(planner, K):
    """Every (vs, type, layout, features, skip regions) at every height 2 .. 700: the choice is the
    reference's, is a build that exists, and a split build's rows tile."""
    NY = range(2, 701)
    keys = list(itertools.product((1, 2), (0, 1), (0, 1), FEATURES, (0, 3)))  # vs, f32, slab, feat, nskip
    lists = {}
    for vs, f32, slab in itertools.product((1, 2), (0, 1), (0, 1)):
        (o,) = planner(["builds %d %d %d" % (f32, vs, slab)])
        lists[vs, f32, slab] = [tuple(b) for b in o["builds"]]
        assert len(set(lists[vs, f32, slab])) == len(lists[vs, f32, slab])
        assert set(lists[vs, f32, slab]) == ref.builds(f32, vs, slab)  # exactly DESIGN §4's table
    outs = planner([choose_line(f32, vs, slab, K, nskip, feat, NY[0], NY[-1]) for vs, f32, slab, feat, nskip in keys])
    for (vs, f32, slab, feat, nskip), o in zip(keys, outs):
        rows, own1 = ref.owned_rows(K, vs), ref.owned_rows(K, 1)
        assert (o["own1"], o["rows_per_wave"], o["ghost"] * vs >= K - 1) == (own1, rows, True)
        assert len(o["c"]) == len(NY)
        for ny, (mode, wpe, nch, top, nin) in zip(NY, o["c"]):
            want = ref.choose(f32, vs, slab, K, ny, nskip, *feat)
            got = dict(mode=mode, wpe=wpe, nch=nch, wall_top=top, wall_ch0=nin)
            assert got == want, (vs, f32, slab, feat, nskip, ny)
            assert (mode, wpe) in lists[vs, f32, slab]
            assert (nch - 1) * rows < ny <= nch * rows
            if mode & ref.SPLIT:
                # bottom chunk [0, own1), inner chunks of `rows` from own1, top chunk [top, ny)
                assert nin >= 1 and top % 2 == 0 and 0 < ny - top <= own1
                assert own1 + (nin - 1) * rows < top <= own1 + nin * rows  # the last inner chunk reaches top, none earlier
            else:
                assert (top, nin) == (0, 0)


# ---- sweeps ----
def sweeps_line(split, vs, cb, ce, step, W, nsweep, nch, nin, slots, wait_lo, wait_hi):
    return "sweeps %d %d %d %d %d %d %d %d %d %d %d %d" % (split, vs, cb, ce, step, W, nsweep, nch, nin, slots, wait_lo, wait_hi)


def check_sweeps(case, o, tiles=True):
    split, vs, cb, ce, step, W, nsweep, nch, nin, slots, wait_lo, wait_hi = case
    families = [(o["ranges"], o["nsweep"])] + ([(o["ranges_w"], o["nsweep_w"])] if split else [])
    for rg, nsw in families:
        assert len(rg) == nsw >= 1
        if tiles:  # non-empty, ordered, and exactly [cb, ce)
            assert rg[0][0] == cb and rg[-1][1] == ce
            assert all(xa < xb for xa, xb in rg) and all(p[1] == q[0] for p, q in zip(rg, rg[1:]))
    if step <= 0:
        assert o["nsweep"] <= ce - cb and o["nsweep_w"] <= ce - cb
    else:
        assert o["nsweep"] == nsweep and o["nsweep_w"] == (nsweep if split else 0)
    assert o["waves"] == (o["nsweep"] * nin + 2 * o["nsweep_w"] if split else o["nsweep"] * nch)
    if step <= 0 and slots > 0:
        assert o["rounds"] >= 1 and o["waves"] <= o["rounds"] * slots
    e = ref.edge_count(o["ranges"], wait_lo, wait_hi)
    ew = ref.edge_count(o["ranges_w"], wait_lo, wait_hi)
    assert o["edge_waves"] == (e * nin + 2 * ew if split else e * nch)


def test_sweeps_random(planner):
    """Balanced sweeps over a seeded random set.  Row chunks as heights up to 700 rows give them (at most
    18); `slots` = 4 waves x blocks per CU x CUs with the CUs a multiple of 8 (the CU masks take whole
    columns of CUs, one of every XCD), so slots >= 32 > nch + 3.  On that domain waves <= rounds * slots
    follows from the floor in the sweep count: plain waves = ns * nch, split at two cells per lane
    ns * (nin + 2); at one cell per lane ns * (nin + 3), plus one wave where ns is odd, which a quotient
    of a multiple of 32 by nin + 3 <= 21 never is when it is exact.  (Outside it that one wave can spill
    into another round: 31 CUs x 12 waves = 372 slots, as IBLB_RESERVE_CUS can leave them, and one inner
    chunk give 93 inner + 2 x 140 wall = 373 waves.  The launch is still correct, and the planner's
    arithmetic is kept as it was.)"""
    rng = np.random.default_rng(20241020)
    cases = []
    for _ in range(3000):
        split, vs = int(rng.integers(2)), int(rng.integers(1, 3))
        nch = int(rng.integers(1, 19))
        nin = int(rng.integers(1, 18)) if split else 0
        cb = int(rng.integers(-8, 50))
        n = int(rng.choice((1, 2, 3, 7, 100, 512, 4096))) if rng.integers(4) == 0 else int(rng.integers(1, 5000))
        W = int(rng.integers(1, 300))
        slots = 0 if rng.integers(8) == 0 else 4 * int(rng.integers(1, 5)) * 8 * int(rng.integers(1, 33))
        lo = int(rng.integers(cb, cb + n + 1))
        wait = (INT_MAX, 0) if rng.integers(6) == 0 else (lo, int(rng.integers(lo, cb + n + 1)))
        cases.append((split, vs, cb, cb + n, 0, W, 32, nch, nin, slots) + wait)
    for c, o in zip(cases, planner([sweeps_line(*c) for c in cases])):
        check_sweeps(c, o)
        if c[9] == 0:  # no occupancy known: the sweeps as requested, clipped at one column each
            n, W = c[3] - c[2], c[5]
            assert o["nsweep"] == min(-(-n // W), n) and o["rounds"] == 0


@pytest.mark.parametrize("split", (0, 1))
def test_sweeps_corners(planner, split):
    nch, nin = 5, 3
    cases = []
    for vs in (1, 2):
        for slots in (0, 256, 1024):
            cases.append((split, vs, 0, 1, 0, 128, 32, nch, nin, slots, INT_MAX, 0))     # one column
            cases.append((split, vs, 0, 5, 0, 1, 32, nch, nin, slots, 2, 3))             # fewer columns than sweeps asked
            cases.append((split, vs, 7, 7 + 4096, 0, 128, 32, nch, nin, slots, 23, 4080))
            # a lone slab's unbalanced form: ceil(ncol / W) fixed sweeps of W columns, the last one clipped
            cases.append((split, vs, 0, 1000, 128, 128, 8, nch, nin, slots, 16, 984))
            cases.append((split, vs, 0, 1024, 128, 128, 8, nch, nin, slots, INT_MAX, 0))
    outs = planner([sweeps_line(*c) for c in cases])
    for c, o in zip(cases, outs):
        check_sweeps(c, o)
    assert outs[0]["nsweep"] == 1 and outs[0]["edge_waves"] == (nin + 2 if split else nch)
    assert outs[1]["nsweep"] == 5
    # a slab's two boundary sweeps, fixed: K columns at each end (the ranges do not tile the slab)
    for K, ncol in ((3, 6), (7, 14), (7, 512)):
        c = (split, 2, 0, ncol, ncol - K, K, 2, nch, nin, 0, INT_MAX, 0)
        (o,) = planner([sweeps_line(*c)])
        check_sweeps(c, o, tiles=False)
        assert o["ranges"] == [[0, K], [ncol - K, ncol]] and o["rounds"] == 0
        assert o["waves"] == o["edge_waves"] == (2 * nin + 4 if split else 2 * nch)


@pytest.mark.parametrize("K", DEPTHS)
def test_edge_waves_slab_interior(planner, K):
    """A slab's interior [K, ncol - K) with wait_lo = 2K + 2, wait_hi = ncol - wait_lo, and every wave an
    edge wave (wait_lo = INT_MAX), on slabs of 2K .. 600 columns: the count is the enumerated one."""
    cases = []
    for ncol in range(2 * K, 601):
        if ncol - 2 * K < 1:
            continue  # no interior column
        lo = 2 * K + 2
        sel = ncol % 4  # every (split, vs) pair in turn, all four at the narrowest and widest slabs
        for split, vs in itertools.product((0, 1), (1, 2)):
            if ncol > 2 * K + 8 and ncol < 592 and 2 * split + vs - 1 != sel:
                continue
            for wait in ((lo, ncol - lo), (INT_MAX, 0)):
                cases.append((split, vs, K, ncol - K, 0, 16 + ncol % 23, 32, 4, 3, (0, 1024)[ncol % 2]) + wait)
    for c, o in zip(cases, planner([sweeps_line(*c) for c in cases])):
        check_sweeps(c, o)
        if c[10] == INT_MAX:
            assert o["edge_waves"] == o["waves"]


# ---- the depths of a call ----
def test_deep_depth(planner):
    outs = planner(["depth %d 0 2000" % K for K in (1, 2, 3) + DEPTHS[1:]])
    for K, o in zip((1, 2, 3) + DEPTHS[1:], outs):
        d = o["d"]
        if K < 4:
            assert set(d) == {K}
            continue
        for r in range(K - 1, 2001):
            pieces, left = ref.call_pieces(K, r, lambda x: d[x])
            assert set(pieces) <= {K - 1, K}
            if r >= (K - 1) * (K - 2):
                assert left == 0 and sum(pieces) == r, (K, r)


# ---- IBLB_DEEP_BUILD ----
def test_parse_deep_build(planner):
    words = ["plain", "split", "pack", "window", "split,window", "window,pack,split", "split,fast", "Plain", "split,"]
    outs = planner(["parse " + w for w in words])
    got = {w: (o["ok"], o["split"], o["pack"], o["window"]) for w, o in zip(words, outs)}
    assert got["plain"] == (1, 0, 0, 0)
    assert got["split"] == (1, 1, 0, 0) and got["pack"] == (1, 0, 1, 0) and got["window"] == (1, 0, 0, 1)
    assert got["split,window"] == (1, 1, 0, 1) and got["window,pack,split"] == (1, 1, 1, 1)
    # an unknown word (an empty one too): refused, the caller's value untouched
    for w in ("split,fast", "Plain", "split,"):
        assert got[w] == (0, 1, 1, 1)
