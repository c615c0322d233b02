"""The IB band planner (csrc/band_plan.h) on the CPU: tests/band_plan_main.cpp, built with
AddressSanitizer + UndefinedBehaviorSanitizer (oracle/Makefile.san), run as a child process over the
point sets of tests/ib_edges.py and a seeded random sweep, and checked against a brute-force model:
boolean cell maps built from the points as the header comment of csrc/ctx_band.hip describes the
cycle, not from the planner's formulas.

Notation: R = 2(K-1), D = gc, m = K-1-j; cover_j = the cells (x, y) with x an entry column of level j
and y in [max(0, pr0 - m), min(ny, pr1 + m)).  Columns are local; the maps hold columns -D-1 ..
ncol+D (index x + D + 1).  Any sanitizer finding aborts the program (-fno-sanitize-recover)."""
import json
import os
import subprocess

import numpy as np
import pytest

import ib_edges

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(REPO, "oracle", "_san", "band_plan_san")
MAX_SKIP = 96


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


def case(K, nx, ny, xy, x_begin=0, ncol=None, edges=(), V=2, f64=0, flux=-1, merged=0, vhalf=0):
    """A planner input; lone slab unless `edges` (the group's slab edges) is given."""
    ncol = nx if ncol is None else ncol
    xy = np.asarray(xy, dtype=np.float32).ravel()
    return dict(K=K, nx=nx, ny=ny, x_begin=x_begin, ncol=ncol, gc=3 * K, slab=int(bool(edges)), V=V, f64=f64,
                flux=flux, merged=merged, vhalf=vhalf, edges=tuple(edges), xy=xy)


def line(c):
    head = [c[k] for k in ("K", "nx", "ny", "x_begin", "ncol", "gc", "slab", "V", "f64", "flux", "merged", "vhalf")]
    pts = " ".join("%.9g" % v for v in c["xy"])
    return "plan %s %d %s %d %s" % (" ".join(map(str, head)), len(c["edges"]), " ".join(map(str, c["edges"])),
                                    c["xy"].size // 2, pts)


def entries(o, j):
    t = o["tab"][o["off"][j]: o["off"][j] + 5 * o["n"][j]]
    return [t[i: i + 5] for i in range(0, len(t), 5)]


def forced_map(c):
    """Item 1's forced cells, every periodic image, and the forced global columns."""
    K, nx, ny, ncol, D = c["K"], c["nx"], c["ny"], c["ncol"], c["gc"]
    F = np.zeros((ncol + 2 * D + 2, ny), dtype=bool)
    gcols = set()
    pts = c["xy"].astype(np.float64).reshape(-1, 2)
    for x0, y0 in np.rint(pts).astype(int):  # ties to even, as nearbyint
        ya, yb = min(max(0, y0 - 1), ny - 1), max(min(ny - 1, y0 + 1), 0)
        for xg in range(x0 - 1, x0 + 2):
            if not 0 <= xg < nx:
                continue
            gcols.add(xg)
            for m in (-1, 0, 1):
                x = xg - c["x_begin"] + m * nx
                if -D + 1 <= x <= ncol + D - 2:
                    F[x + D + 1, ya: yb + 1] = True
    return F, gcols


def dilate(A, r, axis):
    out = A.copy()
    for s in range(1, r + 1):
        for sg in (s, -s):
            sh = np.roll(A, sg, axis=axis)
            idx = [slice(None)] * 2
            idx[axis] = slice(0, s) if sg > 0 else slice(A.shape[axis] - s, None)
            sh[tuple(idx)] = False  # no wrap
            out |= sh
    return out


def check_geometry(c, o):
    """Items 1-4, 6-9 (and the plan's depths); the chunks are check_chunks'."""
    K, nx, ny, ncol, D = c["K"], c["nx"], c["ny"], c["ncol"], c["gc"]
    R, off = 2 * (K - 1), D + 1
    F, gcols = forced_map(c)
    b, pr, d = o["b"], o["pr"], o["d"]
    # 1. forced cells lie in a patch, and the patches are their hulls
    P = np.zeros_like(F)
    for x0, x1, y0, y1 in b:
        assert -D + 1 <= x0 <= x1 <= ncol + D - 2 and 0 <= y0 <= y1 < ny
        P[x0 + off: x1 + off + 1, y0: y1 + 1] = True
        sub = F[x0 + off: x1 + off + 1, y0: y1 + 1]
        assert sub[0].any() and sub[-1].any() and sub[:, 0].any() and sub[:, -1].any()
    assert not (F & ~P).any()
    # 2. patches stay apart
    for p, q in zip(b, b[1:]):
        assert q[0] - p[1] - 1 >= 2 * R + 8
    # the ghost depth: all of D where a level-0 input leaves the slab, else none; the exchange depth
    need = any(x0 - R - 1 < 0 or x1 + R + 1 > ncol - 1 for x0, x1, _, _ in b)
    assert d == (D if need else 0)
    if c["slab"]:
        zone = max(D, R + 2)
        dist = lambda f: min(min(abs(f - e) % nx, nx - abs(f - e) % nx) for e in c["edges"])
        assert o["x"] == max(K, D if any(dist(f) <= zone for f in gcols) else 0)
    else:
        assert o["x"] == 0
    # 3. rows: even bounds (or ny) around the forced rows +- (K-1)
    assert len(pr) == len(b)
    for (x0, x1, y0, y1), (p0, p1) in zip(b, pr):
        assert p0 % 2 == 0 and (p1 % 2 == 0 or p1 == ny) and 0 <= p0 < p1 <= ny
        lo, hi = max(0, y0 - (K - 1)), min(ny, y1 + K)
        assert p0 <= lo < p0 + 2 and (p1 == ny or hi <= p1 < hi + 2)
    # the covers, and the columns the header comment gives each level
    covers = []
    for j in range(K):
        m = K - 1 - j
        C = np.zeros_like(F)
        cols = []
        for x, _, _, p0, p1 in entries(o, j):
            assert [p0, p1] in pr
            C[x + off, max(0, p0 - m): min(ny, p1 + m)] = True
            cols.append((x, p0, p1))
        want = []
        for (x0, x1, _, _), (p0, p1) in zip(b, pr):
            xa, xb = max(x0 - R + j, -d + 1 + j), min(x1 + R - j, ncol + d - 2 - j)
            if j == K - 1:
                xa, xb = max(xa, 0), min(xb, ncol - 1)
            want += [(x, p0, p1) for x in range(xa, xb + 1)]
        assert cols == want
        covers.append(C)
    # 3. exactness: own cells within K-1 of a forced cell are the last level's
    near = dilate(dilate(F, K - 1, 0), K - 1, 1)
    own = np.zeros_like(F)
    own[off: off + ncol] = True
    assert not (near & own & ~covers[K - 1]).any()
    assert not (covers[K - 1] & ~own).any()
    # 4. dependency closure
    for j in range(1, K):
        assert not (dilate(dilate(covers[j], 1, 0), 1, 1) & ~covers[j - 1]).any(), j
    held = np.zeros_like(F)
    held[off - d: off + ncol + d] = True
    assert not (dilate(covers[0], 1, 0) & ~held).any()
    # 6. bookkeeping
    assert len(o["off"]) == len(o["n"]) == len(o["nchl"]) == K and o["off"][0] == 0
    for j in range(K - 1):
        assert o["off"][j + 1] == o["off"][j] + 5 * o["n"][j]
    assert len(o["tab"]) == o["off"][K - 1] + 5 * o["n"][K - 1]
    # 7. skip boxes: the last level's regions, or none
    boxes = []
    for (x0, x1, _, _), (p0, p1) in zip(b, pr):
        xa, xb = max(0, x0 - (K - 1)), min(ncol - 1, x1 + (K - 1))
        if xa <= xb:
            boxes.append([xa, xb, p0, p1])
    S = np.zeros_like(F)
    for xa, xb, p0, p1 in boxes:
        S[xa + off: xb + off + 1, p0: p1] = True
    assert (S == covers[K - 1]).all()
    if len(b) > MAX_SKIP or any(q[0] <= p[1] for p, q in zip(boxes, boxes[1:])):
        boxes = []
    assert o["skip"] == boxes and len(boxes) <= MAX_SKIP
    # 8. flux rows
    hit = [q for q, (x0, x1, _, _) in enumerate(b) if x0 - (K - 1) <= c["flux"] <= x1 + (K - 1)] if c["flux"] >= 0 else []
    if hit:
        assert len(hit) == 1 and [o["flux"], o["fy0"], o["fy1"]] == [c["flux"]] + pr[hit[0]]
    else:
        assert o["flux"] == -1
    # 9. force_clip
    for j in range(K):
        lj, hj = -d + 1 + j, ncol + d - 2 - j  # columns level j can compute
        cl, mg = o["clip_chained"][j], o["clip_merged"][j]
        if j == K - 1:
            assert cl == mg == [max(0, lj), min(ncol, hj + 1)] and 0 <= cl[0] and cl[1] <= ncol
        else:
            assert cl == [lj, hj + 1]
            want = [lj + 1, hj]
            if j == K - 2:
                want = [max(-3, want[0]), min(ncol + 3, want[1])]
            assert mg == want
    # wrap_range: the points near the lattice's x edge, where a ghost trapezoid's slab touches it
    x0 = np.rint(c["xy"][0::2].astype(np.float64)).astype(int)
    margin = D + 2 * K + 4
    near_edge = np.nonzero((x0 < margin) | (x0 > nx - 1 - margin))[0]
    touches = c["x_begin"] == 0 or c["x_begin"] + ncol == nx
    if d > 0 and touches and near_edge.size and near_edge[-1] + 1 - near_edge[0] < x0.size:
        assert o["wrap"] == [near_edge[0], near_edge[-1] + 1]
    else:
        assert o["wrap"] == [0, 0]


def check_chunks(c, o):
    """Items 5 and 6: the row chunks of every entry, nchl and the cell count."""
    K, ny = c["K"], c["ny"]
    U = 64 * c["V"] // (2 if c["vhalf"] else 1)
    cells = 0
    for j in range(K):
        m, tall = K - 1 - j, 0
        for x, ch0, ch1, p0, p1 in entries(o, j):
            ylo, yhi = max(0, p0 - m), min(ny, p1 + m)
            assert ch0 * U <= ylo < (ch0 + 1) * U and (ch1 - 1) * U < yhi <= ch1 * U
            tall = max(tall, ch1 - ch0)
            cells += min(ny, ch1 * U) - ch0 * U
        assert o["nchl"][j] == tall
    assert o["cells"] == cells
    assert o["too_big"] == int(not c["slab"] and 2 * cells > K * c["nx"] * ny)
    assert (o["merged"], o["vhalf"]) == (c["merged"], c["vhalf"])


def same_but_chunks(o, base):
    for k in ("feasible", "d", "x", "b", "pr", "off", "n", "flux", "fy0", "fy1", "skip", "clip_chained",
              "clip_merged", "wrap"):
        assert o[k] == base[k], k
    for i in (0, 3, 4):
        assert o["tab"][i::5] == base["tab"][i::5]


# ---- named inputs: the point sets of tests/ib_edges.py ----
K = ib_edges.K
NX = ib_edges.NX
GROUP = (0, 96, 192, 288)  # a 4-slab group of 96-column slabs


def cycle_points(points, t, k=K):
    """The points of iterations t-1 .. t+k-2 (ctx_band.hip:plan_cycle)."""
    return np.concatenate([points(it)[0] for it in range(t - 1, t + k - 1)])


def named_point_sets():
    out = {}
    for ny in ib_edges.STATIC_NY:  # (static_points gives wall_points at every iteration: one set)
        assert (ib_edges.static_points(NX, ny)(3)[0] == ib_edges.wall_points(NX, ny)[0]).all()
        out[f"wall_{ny}"] = (ny, ib_edges.wall_points(NX, ny)[0])
    sched = ib_edges.moving_schedule(NX, ib_edges.MOVING_NY)
    for t in range(1, ib_edges.MOVING_STEPS - K + 2, K):
        xy = cycle_points(sched, t)
        if xy.size:
            out[f"moving_t{t}"] = (ib_edges.MOVING_NY, xy)
    # a filament across x = 0 (ghost trapezoids on a lone slab) and two filaments 22 columns apart
    # (below 2R + 8 = 32: one patch)
    out["across_x0"] = (131, np.array([(x, 50 + i) for i, x in enumerate((NX - 1.4, NX - 1.0, NX - 0.6, -0.2, 0.3, 0.8))]))
    out["merging"] = (131, np.array([(100.2, 30 + i) for i in range(8)] + [(125.1, 70 + i) for i in range(8)]))
    return out


POINT_SETS = named_point_sets()
VARIANTS = [(2, 0), (2, 1), (4, 0), (4, 1)]  # (V, vhalf)


def placements(ny, xy, **kw):
    yield case(K, NX, ny, xy, **kw)
    for r, e in enumerate(GROUP):
        yield case(K, NX, ny, xy, x_begin=e, ncol=96, edges=GROUP, **kw)


@pytest.mark.parametrize("name", sorted(POINT_SETS))
def test_named_points(planner, name):
    ny, xy = POINT_SETS[name]
    cases = []
    for fi, flux in enumerate((-1, 45, 300)):  # no flux column, one beside the bottom filament, one far from most
        for V, vhalf in (VARIANTS if fi == 0 else VARIANTS[:1]):
            cases += list(placements(ny, xy, V=V, vhalf=vhalf, merged=vhalf ^ 1, flux=flux))
    for c in cases:  # (the flux column is local: where the slab owns it)
        if c["flux"] >= 0:
            f = c["flux"] - c["x_begin"]
            c["flux"] = f if 0 <= f < c["ncol"] else -1
    outs = planner([line(c) for c in cases])
    base = {}
    for c, o in zip(cases, outs):
        assert o["feasible"] and not o["too_big"]
        key = (c["x_begin"], c["ncol"], c["flux"])
        if key not in base:
            check_geometry(c, o)
            base[key] = o
        else:
            same_but_chunks(o, base[key])
        check_chunks(c, o)
    # 10. every rank of the group finds the same exchange depth
    assert len({o["x"] for c, o in zip(cases, outs) if c["slab"]}) == 1
    lone = outs[0]
    if name == "across_x0" or name.startswith("wall"):
        assert lone["d"] > 0  # points in the corners of the lattice
    if name == "merging":
        assert len(lone["b"]) == 1 and lone["b"][0][:2] == [99, 126]


def test_more_patches_than_skip_boxes(planner):
    """Over MAX_SKIP patches: no skip boxes at all, never a truncated list."""
    xy = np.array([(40.0 + 64 * i, 20.0) for i in range(MAX_SKIP + 2)])
    c = case(K, 64 * (MAX_SKIP + 3), 40, xy)
    (o,) = planner([line(c)])
    assert len(o["b"]) == MAX_SKIP + 2 and o["skip"] == []
    check_geometry(c, o)
    check_chunks(c, o)


def test_infeasible_lone_slab(planner):
    """A lone slab narrower than its ghost depth cannot hold a ghost trapezoid's periodic copies."""
    (o,) = planner([line(case(7, 16, 40, [(1.0, 20.0)]))])
    assert not o["feasible"]


def test_random_sweep(planner):
    rng = np.random.default_rng(20240611)
    cases, groups = [], []
    for i in range(400):
        k = int(rng.choice((3, 5, 7)))
        ny = int(rng.choice((40, 131, 257)))
        V, vhalf = VARIANTS[int(rng.integers(3))]  # chunks of 128, 64 or 256 rows
        ranks = int(rng.choice((1, 2, 4)))
        ncol = int(rng.choice((96, 200, 384))) if ranks == 1 else int(rng.integers(4 * k, 4 * k + 41))
        nx = ncol * ranks
        pts = []
        for _ in range(int(rng.integers(1, 5))):  # filaments: a point per row, leaning a little
            n = int(rng.integers(1, 13))
            x, y, lean = rng.uniform(-0.4, nx - 0.6), rng.uniform(-2, ny + 1 - (n - 1)), rng.uniform(-0.3, 0.3)
            pts += [(min(max(x + lean * q, -0.4), nx - 0.6), y + q) for q in range(n)]
        edges = tuple(range(0, nx, ncol)) if ranks > 1 else ()
        flux = int(rng.integers(-1, ncol))
        group = [case(k, nx, ny, pts, x_begin=e, ncol=ncol, edges=edges, V=V, vhalf=vhalf, flux=flux,
                      f64=int(rng.integers(2))) for e in (edges or (0,))]
        groups.append((len(cases), len(group)))
        cases += group
    outs = planner([line(c) for c in cases])
    declined = 0
    for first, n in groups:
        group = list(zip(cases[first: first + n], outs[first: first + n]))
        if any(not o["feasible"] or o["too_big"] for _, o in group):
            declined += 1
            continue
        for c, o in group:
            check_geometry(c, o)
            check_chunks(c, o)
        assert len({o["x"] for _, o in group}) == 1
    assert declined <= 40, declined  # at most 10 % of the cases


def test_arrangement(planner):
    """The three arrangements of DESIGN §5 at depth 7, 32 CUs per XCD, the trapezoids under 5 % of the cycle."""
    lone_f64, lone_f32, slab_f32 = planner([
        "arr 0 1 7 0.01 2048 2048 1 32",             # 2048^2 f64 lone slab: both streams unmasked
        "arr 0 0 7 0.01 8192 2048 1 32",             # 8192 x 2048 f32 lone slab: one XCD's CUs, own build
        "arr 1 0 7 0.01 %d 2048 1 32" % (1024 - 14),  # 1024 x 2048 f32 group slab (its interior): merged, two XCDs'
    ])
    assert lone_f64 == dict(bound=0, merged=0, want=-2, own_build=0)
    assert lone_f32 == dict(bound=0, merged=0, want=32, own_build=1)
    assert slab_f32 == dict(bound=1, merged=1, want=64, own_build=0)
