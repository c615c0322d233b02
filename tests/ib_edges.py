"""Inputs of the IB edge tests (tests/test_gpu_ib_edges.py) and of their envelope
(tests/golden/ib_edge_envelope.json): Lagrangian points on the walls, in the lattice corners, on
half-integer coordinates, and filaments that move across the level launches' row-chunk bounds.

Every other IB test keeps its filaments in mid-lattice on even heights and never moves a point in
y; the band cycle has branches for exactly what those inputs avoid:
* the merged chain's point groups pull the wall rows themselves (bounce-back on row 0, mirror on
  row YDIM-1, csrc/ib_device.h:ib_next_group);
* the planner clips a patch's even row bounds with min(YDIM, ..): odd on an odd height;
* f32 level launches run in 128-row half-chunks that share a flag per 256 rows, never cleared: a
  point that leaves a row relies on the half-chunks zeroing every force row they consumed;
* the reference's flat node index (ImmersedBoundary.cu:119-122) skips nodes with j < 0 (row -1)
  and j >= size (row YDIM), and a node at x = -1 / XDIM reads the neighbouring row.
Test infrastructure (numpy only); the lattices are odd on purpose: 131 rows = one 128-row chunk
plus three ragged rows with the top wall in them, 257 = the top wall alone in its chunk, 601 = five
half-chunks.
"""
import numpy as np

K = 7                                   # the library's default deep-sweep depth (IBLB_SWEEP_DEPTH)
NX = 384
STATIC_NY = (131, 257)
MOVING_NY = 601
STATE_SEED = {131: 7, 257: 7, 601: 13}  # initial-state seeds (chosen by the envelope's cap, see the JSON)
STATIC_STEPS = 1 + 6 * K + 2            # boot, six band cycles, two one-step remainders
PHASE_A = 1 + 8 * K + 1                 # moving points
PHASE_B = 1 + 3 * K                     # points removed: the force owed, then no-IB deep sweeps
PHASE_C = 2 * K + 1                     # a new static filament over two earlier patches
MOVING_STEPS = PHASE_A + PHASE_B + PHASE_C
EPS_OFF_AT = 3 * K + 2                  # the standing filament's epsilon goes to 0 in mid-cycle
SEEDS = (200, 201, 202, 203)            # the envelope's perturbation seeds per magnitude


def _us(n, amp=1e-3, phase=0.0):
    i = np.arange(n)
    us = np.empty(2 * n, dtype=np.float32)
    us[0::2] = amp * np.sin(0.7 * i + phase)
    us[1::2] = -0.3 * amp * np.cos(0.4 * i + phase)
    return us


def wall_points(nx, ny):
    """41 static points, each group for one edge (s, u_s float32 xy interleaved, epsilon int32)."""
    f32 = np.float32
    xy = []
    # bottom filament: y0 = 0 (node row -1 skipped by j < 0; bounce-back pulls on row 0), 14 points
    xy += [(40.3 + 0.2 * np.sin(0.9 * i), y) for i, y in enumerate([0.0, 0.4] + list(range(1, 13)))]
    # top filament: y0 = YDIM-1 (node row YDIM skipped by j >= size; mirror pulls), 13 points
    xy += [(120.6 + 0.2 * np.cos(0.8 * i), ny - 1 - d) for i, d in enumerate([0.0, 0.45] + list(range(1, 12)))]
    # corner x0 = 0, y0 = 0: node (-1, 0) has j = -1 (skipped), node (-1, 1) reads (XDIM-1, 0)
    xy += [(0.2, 0.3), (0.2, 1.2), (0.3, 2.2), (0.4, 3.3)]
    # corner x0 = XDIM-1, y0 = YDIM-1: node (XDIM, YDIM-1) has j = size (skipped), (XDIM, YDIM-2) reads (0, YDIM-1)
    xy += [(nx - 0.7, ny - 1.2), (nx - 0.7, ny - 2.3), (nx - 0.6, ny - 3.3), (nx - 0.8, ny - 4.4)]
    # half-integers and one float ulp to either side, in x and y: ties-to-even of nearbyint, delta at |d| = 1.5
    xy += [(200.5, 60.5), (201.5, 61.5),
           (np.nextafter(f32(202.5), f32(0)), np.nextafter(f32(62.5), f32(0))),
           (np.nextafter(f32(203.5), f32(np.inf)), np.nextafter(f32(63.5), f32(np.inf)))]
    # two coincident points: both atomics land in the same cells
    xy += [(280.37, 30.6), (280.37, 30.6)]
    s = np.array(xy, dtype=np.float32).ravel()
    n = s.size // 2
    eps = np.ones(n, dtype=np.int32)
    eps[[5, 14 + 3, 14 + 13 + 8 + 1]] = 0  # one on each wall filament and a half-integer point
    return s, _us(n), eps


def static_points(nx, ny):
    """points(it) of a static configuration (the same arrays every iteration)."""
    pts = wall_points(nx, ny)
    return lambda it: pts


# columns of the five moving filaments (>= 60 apart: the planner keeps five patches) and their first rows
_FIL_X = (40.3, 110.6, 180.2, 250.7, 330.4)
_NPTS = 24


def moving_points(nx, ny):
    """points(it), it < PHASE_A: five 24-point filaments swaying +-1.5 columns; u_s ~ 1e-3, independent of
    the motion.  In the order of the points:
    0 sinks 0.75 rows per iteration until its lowest points sit clipped on row 0 (two on the wall, one
      0.75 above: it stops sinking there; more points stacked in one cell over-correct the reference's
      penalty force, workloads.filament) — from iteration 38 on;
    1 rises 0.75 rows per iteration across row 256 (the f32 flag-chunk bound);
    2 rises across row 128 (the f32 half-chunk bound, the f64 chunk bound);
    3 rises until its top points sit clipped on YDIM-1 (likewise two), from iteration 40;
    4 stands still; its epsilon goes to 0 at iteration EPS_OFF_AT."""
    k = np.arange(_NPTS, dtype=np.float64)
    us = np.concatenate([_us(_NPTS, 1e-3, 0.5 * m) for m in range(5)])

    def points(it):
        s = np.empty((5, _NPTS, 2), dtype=np.float64)
        for m, xc in enumerate(_FIL_X):
            s[m, :, 0] = xc + 1.5 * (0.3 + 0.7 * k / (_NPTS - 1)) * np.sin(2 * np.pi * (it + 4 * m) / 19.0)
        d = 0.75 * it
        s[0, :, 1] = np.maximum(28.25 + k - min(d, 29.5), 0.0)
        s[1, :, 1] = 225.3 + k + d
        s[2, :, 1] = 95.6 + k + d
        s[3, :, 1] = np.minimum(ny - 1 - 52.75 + k + min(d, 31.0), ny - 1)
        s[4, :, 1] = 300.4 + k
        eps = np.ones(5 * _NPTS, dtype=np.int32)
        eps[np.arange(5 * _NPTS) % 9 == 4] = 0
        if it >= EPS_OFF_AT:
            eps[4 * _NPTS:] = 0
        return s.astype(np.float32).ravel(), us, eps
    return points


def return_points(nx, ny):
    """Phase C: a static slanted filament from the columns of filament 1's patch to those of filament 2's,
    across row 256 (80 points, spacing 1.2)."""
    k = np.arange(80, dtype=np.float64)
    s = np.empty(160, dtype=np.float32)
    s[0::2] = 107.4 + 0.97 * k
    s[1::2] = 225.5 + 0.7 * k
    return s, _us(80, 1e-3, 0.3), (np.arange(80) % 11 != 6).astype(np.int32)


_NONE = (np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))


def moving_schedule(nx, ny):
    """points(it) over the whole moving configuration: phase A (moving), B (no points), C (return_points)."""
    a, c = moving_points(nx, ny), return_points(nx, ny)

    def points(it):
        return a(it) if it < PHASE_A else _NONE if it < PHASE_A + PHASE_B else c
    return points


# name: (nx, ny, initial-state seed, iterations, points(it), iterations after which the fields are compared)
def configs():
    out = {}
    for ny in STATIC_NY:
        out[f"static_{NX}x{ny}"] = (NX, ny, STATE_SEED[ny], STATIC_STEPS, static_points(NX, ny), (STATIC_STEPS,))
    out[f"moving_{NX}x{MOVING_NY}"] = (NX, MOVING_NY, STATE_SEED[MOVING_NY], MOVING_STEPS,
                                       moving_schedule(NX, MOVING_NY),
                                       (PHASE_A, PHASE_A + PHASE_B, MOVING_STEPS))
    return out
