"""Host-side mirror of the fused context API (include/iblb.h, part 2).

`Lattice` owns one x-slab of a D2Q9 channel on one GPU and advances the reference time step
(main.cu:852-909: equilibrium -> collision -> streaming -> macro -> interpolate -> spread).
Arrays crossing this boundary are numpy arrays in the reference layouts restricted to the
slab: rho[N], u[2N] (u_x block then u_y block), force[2N], f[9N] AoS (f[9*j+i]),
j = y * x_count + (x - x_begin); Lagrangian s/u_s interleaved float32 xy, epsilon int32.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass

import numpy as np

from . import _lib as L


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _addr(a: np.ndarray | None):
    """The address of a's data for a pointer member of a ctypes struct (None: NULL); the caller keeps `a` alive."""
    return None if a is None else a.ctypes.data


def _window(w):
    """None, an L.Window or (x0, y0, nx, ny, sx, sy) as an L.Window (or None)."""
    if w is None or isinstance(w, L.Window):
        return w
    x0, y0, nx, ny, sx, sy = (int(v) for v in w)
    return L.Window(x0, y0, nx, ny, sx, sy)


@dataclass
class Stats:
    """One quantity's iblb_field_stats, plus its row sums [window ny] and column sums [nx_local]
    (None where not asked for).  Indices are window sample indices; count == 0: min / max = +inf /
    -inf and the indices -1."""
    count: int = 0
    nonfinite: int = 0
    sum: float = 0.0
    sum_sq: float = 0.0
    min: float = math.inf
    max: float = -math.inf
    min_i: int = -1
    min_j: int = -1
    max_i: int = -1
    max_j: int = -1
    row_sum: np.ndarray | None = None
    col_sum: np.ndarray | None = None


def combine_stats(parts):
    """Merge per-slab results of Lattice.reduce, given in slab order (left to right): a list of
    {name: Stats} gives {name: Stats}, a list of Stats one Stats.  Counts and sums add; min / max
    keep the lower / higher value and, among equal values, the sample with the lowest j, then the
    lowest i (iblb_reduce_fields' tie rule); row sums add; column sums concatenate."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_stats needs at least one part")
    if isinstance(parts[0], dict):
        return {n: combine_stats([p[n] for p in parts]) for n in parts[0]}
    out = Stats()
    for p in parts:
        out.count += p.count
        out.nonfinite += p.nonfinite
        out.sum += p.sum
        out.sum_sq += p.sum_sq
        if p.count > 0:
            if p.min < out.min or (p.min == out.min and (p.min_j, p.min_i) < (out.min_j, out.min_i)):
                out.min, out.min_i, out.min_j = p.min, p.min_i, p.min_j
            if p.max > out.max or (p.max == out.max and (p.max_j, p.max_i) < (out.max_j, out.max_i)):
                out.max, out.max_i, out.max_j = p.max, p.max_i, p.max_j
    if all(p.row_sum is not None for p in parts):
        out.row_sum = np.sum([p.row_sum for p in parts], axis=0)
    if all(p.col_sum is not None for p in parts):
        out.col_sum = np.concatenate([p.col_sum for p in parts])
    return out


# ---- reference parameter derivation (main.cu:296-321) -------------------------------------

C_S_DRIVER = 0.577  # main.cu:27 (the kernels use 0.57735, LatticeBoltzmann.cu:11)
LENGTH = 96         # main.cu:279
YDIM_REF = 192      # main.cu:271


@dataclass
class RefParams:
    """Derived run parameters of the reference driver for its 10 positional arguments."""
    c_fraction: int
    c_num: int
    c_space: int
    Re: float
    T_num: float
    T_pow: int
    I_pow: float
    P_num: int
    ShARC: bool
    BigData: bool

    @property
    def XDIM(self) -> int:  # main.cu:298
        return self.c_num * self.c_space

    @property
    def YDIM(self) -> int:
        return YDIM_REF

    @property
    def T(self) -> int:  # main.cu:299
        return int(np.rint(np.float32(self.T_num) * 10.0 ** self.T_pow))

    @property
    def ITERATIONS(self) -> int:  # main.cu:300 (unsigned int = T * float I_pow, truncated)
        return int(self.T * np.float32(self.I_pow))

    @property
    def INTERVAL(self) -> int:  # main.cu:301
        return self.ITERATIONS // self.P_num

    @property
    def SPEED(self) -> float:  # main.cu:314
        return 0.8 * 1000 / self.T

    @property
    def TAU(self) -> float:  # main.cu:320
        return (self.SPEED * LENGTH) / (self.Re * C_S_DRIVER * C_S_DRIVER) + 1. / 2.

    @property
    def TAU2(self) -> float:  # main.cu:321
        return 1. / (12. * (self.TAU - (1. / 2.))) + (1. / 2.)


def reference_taus(Re: float = 1.0, T: int = 100000) -> tuple[float, float]:
    """TAU, TAU2 of main.cu:314-321 for a Reynolds number and beat period."""
    speed = 0.8 * 1000 / T
    tau = (speed * LENGTH) / (Re * C_S_DRIVER * C_S_DRIVER) + 0.5
    return tau, 1. / (12. * (tau - 0.5)) + 0.5


def plan_slabs(nx: int, n: int) -> list[tuple[int, int]]:
    """x-slab decomposition: n contiguous column ranges covering [0, nx) in order."""
    if n < 1 or n > nx:
        raise ValueError(f"cannot split {nx} columns into {n} slabs")
    edges = [(r * nx) // n for r in range(n + 1)]
    return [(edges[r], edges[r + 1] - edges[r]) for r in range(n)]


class Lattice:
    """One slab (or the whole lattice) on one GPU, behind the C ABI."""

    def __init__(self, nx: int, ny: int, tau: float | None = None, tau2: float | None = None, *,
                 precision: str = "f64", body_force=(0.0, 0.0), flux_norm: float = 192.0,
                 flux_column: int | None = None, device: int = 0, x_begin: int = 0, x_count: int = 0,
                 max_points: int = 0, lib=None):
        lib = lib or L.load()
        self._lib = lib
        cfg = L.Config()
        L.check(lib.iblb_config_default(C.byref(cfg)))
        if tau is None:
            tau, tau2 = reference_taus()
        cfg.nx, cfg.ny = int(nx), int(ny)
        cfg.tau, cfg.tau2 = float(tau), float(tau2)
        if precision not in ("f64", "f32"):
            raise ValueError("precision must be 'f64' or 'f32'")
        cfg.precision = L.PREC_F64 if precision == "f64" else L.PREC_F32
        cfg.body_force[0], cfg.body_force[1] = float(body_force[0]), float(body_force[1])
        cfg.flux_norm = float(flux_norm)
        cfg.flux_column = int(nx) - 5 if flux_column is None else int(flux_column)
        cfg.device = int(device)
        cfg.x_begin, cfg.x_count = int(x_begin), int(x_count)
        cfg.max_points = int(max_points)
        h = C.c_void_p()
        rc = lib.iblb_create(C.byref(cfg), C.byref(h))
        L.check(rc, None, lib)
        self._h = h
        self.nx, self.ny = int(nx), int(ny)
        self.x_begin = int(x_begin) if x_count > 0 else 0
        self.x_count = int(x_count) if x_count > 0 else int(nx)
        self.N = self.x_count * self.ny
        self.precision = precision
        self.max_points = int(max_points)
        self.ns = 0

    # -- lifecycle ------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.iblb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int) -> None:
        L.check(rc, self._h, self._lib)

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    # -- state ------------------------------------------------------------------------------
    def set_state(self, rho=None, u=None, f=None, force=None) -> None:
        def arr(a, n):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != n:
                raise ValueError(f"expected {n} values, got {a.size}")
            return a
        rho, u = arr(rho, self.N), arr(u, 2 * self.N)
        f, force = arr(f, 9 * self.N), arr(force, 2 * self.N)
        if (rho is None) != (u is None):
            rho = np.ones(self.N) if rho is None else rho
            u = np.zeros(2 * self.N) if u is None else u
        self._check(self._lib.iblb_set_state(self._h, _ptr(rho), _ptr(u), _ptr(f), _ptr(force)))

    def set_lagrangian(self, s, u_s, epsilon=None) -> None:
        s = np.ascontiguousarray(s, dtype=np.float32).ravel()
        u_s = np.ascontiguousarray(u_s, dtype=np.float32).ravel()
        ns = s.size // 2
        if u_s.size != 2 * ns:
            raise ValueError("s and u_s must both hold 2*Ns values")
        eps = None if epsilon is None else np.ascontiguousarray(epsilon, dtype=np.int32).ravel()
        self._check(self._lib.iblb_set_lagrangian(self._h, ns, _ptr(s), _ptr(u_s), _ptr(eps)))
        self.ns = ns

    def set_lagrangian_steps(self, s, u_s, epsilon=None) -> None:
        """Points of the next n iterations given ahead (iblb_set_lagrangian_steps): s, u_s of
        shape (n, 2*Ns) (float32 xy), epsilon (n, Ns) or None; iteration steps+i uses row i."""
        s = np.ascontiguousarray(s, dtype=np.float32)
        u_s = np.ascontiguousarray(u_s, dtype=np.float32)
        if s.ndim != 2 or s.shape != u_s.shape or s.shape[1] % 2:
            raise ValueError("s and u_s must both have shape (nsteps, 2*Ns)")
        n, ns = s.shape[0], s.shape[1] // 2
        eps = None
        if epsilon is not None:
            eps = np.ascontiguousarray(epsilon, dtype=np.int32)
            if eps.shape != (n, ns):
                raise ValueError("epsilon must have shape (nsteps, Ns)")
        self._check(self._lib.iblb_set_lagrangian_steps(self._h, n, ns, _ptr(s), _ptr(u_s), _ptr(eps)))
        self.ns = ns

    def set_cilia(self, c_num: int, c_space: float, T: int, p_step: int) -> None:
        """Run the reference's cilia kinematics on the device every iteration (main.cu:822-841);
        c_num = 0 switches it off.  Needs max_points >= 96 * c_num."""
        k = L.Cilia(int(c_num), float(c_space), int(T), int(p_step))
        self._check(self._lib.iblb_set_cilia(self._h, C.byref(k)))
        self.ns = 96 * int(c_num) if c_num > 0 else 0

    def lagrangian(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Current Lagrangian points: s [2Ns], u_s [2Ns] (float32), epsilon [Ns] (int32)."""
        s = np.zeros(2 * self.ns, dtype=np.float32)
        us = np.zeros(2 * self.ns, dtype=np.float32)
        eps = np.zeros(self.ns, dtype=np.int32)
        self._check(self._lib.iblb_get_lagrangian(self._h, _ptr(s), _ptr(us), _ptr(eps)))
        return s, us, eps

    def step(self, n: int = 1) -> None:
        self._check(self._lib.iblb_step(self._h, int(n)))

    # -- readers ----------------------------------------------------------------------------
    def macro(self) -> tuple[np.ndarray, np.ndarray]:
        rho = np.empty(self.N)
        u = np.empty(2 * self.N)
        self._check(self._lib.iblb_get_macro(self._h, _ptr(rho), _ptr(u)))
        return rho, u

    def populations(self) -> np.ndarray:
        f = np.empty(9 * self.N)
        self._check(self._lib.iblb_get_populations(self._h, _ptr(f)))
        return f

    def force(self) -> np.ndarray:
        out = np.empty(2 * self.N)
        self._check(self._lib.iblb_get_force(self._h, _ptr(out)))
        return out

    def lagrangian_force(self) -> np.ndarray:
        out = np.zeros(2 * self.ns, dtype=np.float32)
        self._check(self._lib.iblb_get_lagrangian_force(self._h, _ptr(out)))
        return out

    @property
    def flux(self) -> float:
        q = C.c_double(0.0)
        self._check(self._lib.iblb_get_flux(self._h, C.byref(q)))
        return q.value

    def window_local(self, window=None) -> tuple[int, int]:
        """(i_first, nx_local): the samples of `window` whose column this slab owns
        (iblb_window_local).  window: None (whole lattice), an L.Window or (x0, y0, nx, ny, sx, sy)."""
        w = _window(window)
        i0, n = C.c_int(0), C.c_int(0)
        self._check(self._lib.iblb_window_local(self._h, None if w is None else C.byref(w), C.byref(i0), C.byref(n)))
        return i0.value, n.value

    def fields(self, names, window=None) -> dict:
        """Fields on a strided window, computed on the device and copied out at the window's size
        (iblb_get_fields).  names: any of "rho", "ux", "uy", "vort", "sxx", "sxy", "syy" and, with a
        scalar set, "c", "cux", "cuy" (L.READ_FIELDS; C as `scalar` returns it, C*ux, C*uy); returns
        {name: array (ny, nx_local)} of this slab's samples (collective in an RCCL group)."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [n for n in names if n not in L.READ_FIELDS]
        if unknown or not names:
            raise ValueError(f"fields must be chosen from {sorted(L.READ_FIELDS)}, got {names}")
        w = _window(window)
        _, nxl = self.window_local(w)
        ny = self.ny if w is None else w.ny
        order = sorted(set(names), key=L.READ_FIELDS.get)
        bits = sum(L.READ_FIELDS[n] for n in order)
        out = np.empty((len(order), ny, nxl))
        self._check(self._lib.iblb_get_fields(self._h, None if w is None else C.byref(w), bits, _ptr(out)))
        return {n: out[k] for k, n in enumerate(order)}

    def reduce(self, names, window=None, rows=False, cols=False) -> dict:
        """Statistics of quantities over a strided window, reduced on the device (iblb_reduce_fields):
        nothing of the window's size is copied.  names: any of L.QUANTITIES (the fields of `fields`
        plus "momx", "momy", "ke", "usq"; "c", "cux", "cuy" last); returns {name: Stats} in ascending bit order, for this
        slab's samples (collective in an RCCL group).  rows / cols: also the sums over this slab's i
        of every window row (Stats.row_sum) / over j of every sample column (Stats.col_sum)."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [n for n in names if n not in L.QUANTITIES]
        if unknown or not names:
            raise ValueError(f"quantities must be chosen from {sorted(L.QUANTITIES)}, got {names}")
        w = _window(window)
        _, nxl = self.window_local(w)
        ny = self.ny if w is None else w.ny
        order = sorted(set(names), key=L.QUANTITIES.get)
        bits = sum(L.QUANTITIES[n] for n in order)
        st = (L.FieldStats * len(order))()
        rs = np.zeros((len(order), ny)) if rows else None
        cs = np.zeros((len(order), nxl)) if cols else None
        self._check(self._lib.iblb_reduce_fields(self._h, None if w is None else C.byref(w), bits, st, _ptr(rs),
                                                 _ptr(cs)))
        return {n: Stats(*(getattr(st[k], f) for f, _ in L.FieldStats._fields_),
                         row_sum=rs[k] if rows else None, col_sum=cs[k] if cols else None)
                for k, n in enumerate(order)}

    def sample(self, names, x, y) -> dict:
        """Fields at arbitrary points, bilinearly interpolated on the device (iblb_sample_points).
        names as for `fields`; x, y: global lattice coordinates, 0 <= x < nx (periodic), 0 <= y <= ny-1.
        Returns {name: array [n]} in ascending bit order.  A lone slab only."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [n for n in names if n not in L.READ_FIELDS]
        if unknown or not names:
            raise ValueError(f"fields must be chosen from {sorted(L.READ_FIELDS)}, got {names}")
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        if x.size != y.size:
            raise ValueError("x and y must hold the same number of points")
        order = sorted(set(names), key=L.READ_FIELDS.get)
        bits = sum(L.READ_FIELDS[n] for n in order)
        out = np.empty((len(order), x.size))
        self._check(self._lib.iblb_sample_points(self._h, x.size, _ptr(x), _ptr(y), bits, _ptr(out)))
        return {n: out[k] for k, n in enumerate(order)}

    # -- passive tracers ----------------------------------------------------------------------
    def set_tracers(self, x, y, stride: int = 1) -> None:
        """Tracers at (x, y) that `step` moves with the fluid: one explicit-Euler update every
        `stride` iterations (iblb_set_tracers).  Empty x, y remove them.  A lone slab only."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        if x.size != y.size:
            raise ValueError("x and y must hold the same number of tracers")
        self._check(self._lib.iblb_set_tracers(self._h, x.size, _ptr(x), _ptr(y), int(stride)))

    def tracer_info(self) -> dict:
        """{"n", "stride", "updates"} of the tracers (iblb_tracer_count); n == 0: none set."""
        n, stride, updates = C.c_longlong(0), C.c_int(0), C.c_longlong(0)
        self._check(self._lib.iblb_tracer_count(self._h, C.byref(n), C.byref(stride), C.byref(updates)))
        return {"n": n.value, "stride": stride.value, "updates": updates.value}

    def tracers(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Current tracers: x [n], y [n] (float64) and laps [n] (int32), the wraps in x counted so
        that the net x displacement is x - x_start + laps * nx."""
        n = self.tracer_info()["n"]
        x, y, laps = np.empty(n), np.empty(n), np.zeros(n, dtype=np.int32)
        self._check(self._lib.iblb_get_tracers(self._h, _ptr(x), _ptr(y), _ptr(laps)))
        return x, y, laps

    # -- the tracers' motion model: particles -----------------------------------------------------
    def set_tracer_model(self, diffusivity: float = 0.0, drift=(0, 0), walls=("clamp", "clamp"), seed: int = 0,
                         status=None, iteration=None) -> None:
        """Particles: the current tracers also jitter (a uniform random step of variance 2 * diffusivity *
        stride per update), settle with the velocity `drift` and meet the bottom and top wall as `walls` says
        ("clamp", "reflect" or "absorb": the tracer deposits and never moves again) (iblb_set_tracer_model).
        status, iteration: the fates to start from, as `tracer_fates` returned them; neither: all alive."""
        unknown = [w for w in walls if w not in L.TRACER_WALLS]
        if unknown or len(walls) != 2:
            raise ValueError(f"walls must be two of {sorted(L.TRACER_WALLS)}, got {walls}")
        m = L.TracerModel(float(diffusivity), (C.c_double * 2)(float(drift[0]), float(drift[1])),
                          (C.c_int * 2)(L.TRACER_WALLS[walls[0]], L.TRACER_WALLS[walls[1]]), int(seed) & (2**64 - 1))
        st = None if status is None else np.ascontiguousarray(status, dtype=np.int32).ravel()
        it = None if iteration is None else np.ascontiguousarray(iteration, dtype=np.int64).ravel()
        n = self.tracer_info()["n"]
        if any(a is not None and a.size != n for a in (st, it)):
            raise ValueError(f"status and iteration must hold one entry per tracer ({n})")
        self._check(self._lib.iblb_set_tracer_model(self._h, C.byref(m), _ptr(st), _ptr(it)))

    def remove_tracer_model(self) -> None:
        """The tracers take the plain update again (iblb_set_tracer_model with no model)."""
        self._check(self._lib.iblb_set_tracer_model(self._h, None, None, None))

    def tracer_model_info(self) -> dict:
        """{"present", "diffusivity", "drift", "walls", "seed", "alive", "at_bottom", "at_top"} of the tracers'
        model (iblb_tracer_model_info); present False: none set."""
        m, present, counts = L.TracerModel(), C.c_int(0), (C.c_longlong * 3)()
        self._check(self._lib.iblb_tracer_model_info(self._h, C.byref(m), C.byref(present), counts))
        names = {v: k for k, v in L.TRACER_WALLS.items()}
        return {"present": bool(present.value), "diffusivity": m.diffusivity, "drift": (m.drift[0], m.drift[1]),
                "walls": (names[m.wall[0]], names[m.wall[1]]), "seed": m.seed,
                "alive": counts[0], "at_bottom": counts[1], "at_top": counts[2]}

    def tracer_fates(self) -> tuple[np.ndarray, np.ndarray]:
        """status [n] (int32: 0 alive, 1 at the bottom, 2 at the top) and the hit iteration [n] (int64, -1 while
        alive) of the tracers under a model (iblb_get_tracer_fates)."""
        n = self.tracer_info()["n"]
        status, iteration = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int64)
        self._check(self._lib.iblb_get_tracer_fates(self._h, _ptr(status), _ptr(iteration)))
        return status, iteration

    def tracer_deposits(self) -> tuple[np.ndarray, np.ndarray]:
        """bottom [nx], top [nx] (int64): the deposited tracers of each wall per column floor(x), counted on
        the device (iblb_get_tracer_deposits)."""
        bottom, top = np.zeros(self.nx, dtype=np.int64), np.zeros(self.nx, dtype=np.int64)
        self._check(self._lib.iblb_get_tracer_deposits(self._h, _ptr(bottom), _ptr(top)))
        return bottom, top

    # -- time- and phase-averaged fields --------------------------------------------------------
    def set_average(self, names, window=None, stride: int = 1, nbins: int = 1, squares: bool = False,
                    uxuy: bool = False) -> None:
        """Sums of the named fields over `window` that `step` accumulates on the device: one sample
        every `stride` iterations, sample m into bin m % nbins (iblb_set_average).  squares: also the
        sums of v*v; uxuy: also the sum of ux*uy (needs "ux" and "uy").  Empty names remove
        averaging.  A lone slab only."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [n for n in names if n not in L.READ_FIELDS]
        if unknown:
            raise ValueError(f"fields must be chosen from {sorted(L.READ_FIELDS)}, got {names}")
        if not names:
            self._check(self._lib.iblb_set_average(self._h, None, 0, 1, 1, 0))
            return
        w = _window(window)
        bits = sum(L.READ_FIELDS[n] for n in set(names))
        flags = (L.AVG_SQ if squares else 0) | (L.AVG_UXUY if uxuy else 0)
        self._check(self._lib.iblb_set_average(self._h, None if w is None else C.byref(w), bits, int(stride),
                                               int(nbins), flags))

    def reset_average(self) -> None:
        """Zero the sums and counts; the next sample is number 0, `stride` iterations from now
        (iblb_reset_average)."""
        self._check(self._lib.iblb_reset_average(self._h))

    def average_info(self) -> dict:
        """{"window": (x0, y0, nx, ny, sx, sy), "fields", "names", "stride", "nbins", "flags",
        "samples_total"} of the averaging (iblb_average_info); fields == 0: none set."""
        w, fields, stride, nbins = L.Window(), C.c_uint(0), C.c_int(0), C.c_int(0)
        flags, total = C.c_uint(0), C.c_longlong(0)
        self._check(self._lib.iblb_average_info(self._h, C.byref(w), C.byref(fields), C.byref(stride), C.byref(nbins),
                                                C.byref(flags), C.byref(total)))
        return {"window": (w.x0, w.y0, w.nx, w.ny, w.sx, w.sy), "fields": fields.value,
                "names": [n for n, b in L.READ_FIELDS.items() if fields.value & b], "stride": stride.value,
                "nbins": nbins.value, "flags": flags.value, "samples_total": total.value}

    def average(self, bin: int = 0) -> dict:
        """The raw sums of one bin (iblb_get_average): {"samples": n, "sum": {name: (ny, nx)},
        "sum_sq": {name: (ny, nx)} or None, "sum_uxuy": (ny, nx) array or None}, names in ascending
        bit order."""
        info = self.average_info()
        if not info["fields"]:
            self._check(self._lib.iblb_get_average(self._h, int(bin), None, None, None, None))
        order = info["names"]
        nx, ny = info["window"][2], info["window"][3]
        s = np.empty((len(order), ny, nx))
        sq = np.empty((len(order), ny, nx)) if info["flags"] & L.AVG_SQ else None
        xy = np.empty((ny, nx)) if info["flags"] & L.AVG_UXUY else None
        n = C.c_longlong(0)
        self._check(self._lib.iblb_get_average(self._h, int(bin), _ptr(s), _ptr(sq), _ptr(xy), C.byref(n)))
        return {"samples": n.value, "sum": {m: s[k] for k, m in enumerate(order)},
                "sum_sq": None if sq is None else {m: sq[k] for k, m in enumerate(order)}, "sum_uxuy": xy}

    def mean(self, bin: int = 0) -> dict:
        """{name: sum / samples} of one bin (NaN where the bin holds no sample)."""
        a = self.average(bin)
        with np.errstate(invalid="ignore", divide="ignore"):
            return {m: v / float(a["samples"]) for m, v in a["sum"].items()}

    # -- history: probe time series and tracer pathlines ------------------------------------------
    def set_history(self, names=(), x=None, y=None, stride: int = 1, capacity: int = 1024,
                    follow_tracers: bool = False) -> None:
        """A record of the named fields at the probes (x, y) every `stride` iterations, kept in a ring of
        `capacity` records on the device with running statistics per probe (iblb_set_history).
        follow_tracers: the probes are the current tracers, x and y are ignored, every record also holds their
        x, y and laps, and names may be empty (positions only).  A lone slab only; one history per lattice."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [n for n in names if n not in L.READ_FIELDS]
        if unknown:
            raise ValueError(f"fields must be chosen from {sorted(L.READ_FIELDS)}, got {names}")
        bits = sum(L.READ_FIELDS[n] for n in set(names))
        if follow_tracers:
            self._check(self._lib.iblb_set_history(self._h, 0, None, None, bits, int(stride), int(capacity),
                                                   L.HIST_TRACERS))
            return
        if x is None or y is None:
            raise ValueError("x and y are needed unless follow_tracers is set")
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        if x.size != y.size or x.size == 0:
            raise ValueError("x and y must hold the same number of probes, at least one (remove_history removes)")
        self._check(self._lib.iblb_set_history(self._h, x.size, _ptr(x), _ptr(y), bits, int(stride), int(capacity), 0))

    def remove_history(self) -> None:
        """Remove the history; `step` is then what it is without one."""
        self._check(self._lib.iblb_set_history(self._h, 0, None, None, 0, 1, 1, 0))

    def reset_history(self) -> None:
        """Zero the record count and the statistics and keep the probes; the next record is number 0,
        `stride` iterations from now (iblb_reset_history)."""
        self._check(self._lib.iblb_reset_history(self._h))

    def history_info(self) -> dict:
        """{"n", "fields", "names", "stride", "capacity", "flags", "follow_tracers", "recorded", "planes"} of the
        history (iblb_history_info); n == 0: none set.  planes: the plane names of a record in order."""
        n, fields, stride = C.c_longlong(0), C.c_uint(0), C.c_int(0)
        cap, flags, rec = C.c_longlong(0), C.c_uint(0), C.c_longlong(0)
        self._check(self._lib.iblb_history_info(self._h, C.byref(n), C.byref(fields), C.byref(stride), C.byref(cap),
                                                C.byref(flags), C.byref(rec)))
        names = [m for m, b in L.READ_FIELDS.items() if fields.value & b]
        follow = bool(flags.value & L.HIST_TRACERS)
        return {"n": n.value, "fields": fields.value, "names": names, "stride": stride.value, "capacity": cap.value,
                "flags": flags.value, "follow_tracers": follow, "recorded": rec.value,
                "planes": (["x", "y", "laps"] if follow else []) + names if n.value else []}

    def history(self, first=None, count=None) -> dict:
        """Records [first, first + count) of the ring (iblb_get_history): {"iteration": (count,) int64, name:
        (count, n) per recorded field, and "x", "y", "laps" (laps as float64) when following tracers}.  By
        default everything the ring still holds; first alone: from there to the newest record."""
        info = self.history_info()
        if not info["n"]:
            self._check(self._lib.iblb_get_history(self._h, 0, 0, None, None))
        oldest = max(0, info["recorded"] - info["capacity"])
        first = oldest if first is None else int(first)
        count = info["recorded"] - first if count is None else int(count)
        planes, n = info["planes"], info["n"]
        out = np.empty((max(count, 0), len(planes), n))
        it = np.zeros(max(count, 0), dtype=np.int64)
        if count == 0 and oldest <= first <= info["recorded"]:
            return {"iteration": it, **{m: out[:, k, :] for k, m in enumerate(planes)}}
        self._check(self._lib.iblb_get_history(self._h, first, count, _ptr(out), _ptr(it)))
        return {"iteration": it, **{m: out[:, k, :] for k, m in enumerate(planes)}}

    def history_stats(self) -> dict:
        """The running statistics over every record since the set or the last reset (iblb_get_history_stats):
        {plane name: {"count", "nonfinite", "sum", "sum_sq", "min", "max", "min_rec", "max_rec"}}, each [n]."""
        info = self.history_info()
        if not info["n"]:
            self._check(self._lib.iblb_get_history_stats(self._h, None, None, None, None, None, None, None, None))
        planes, n = info["planes"], info["n"]
        kinds = {"count": np.int64, "nonfinite": np.int64, "sum": np.float64, "sum_sq": np.float64,
                 "min": np.float64, "max": np.float64, "min_rec": np.int64, "max_rec": np.int64}
        arr = {k: np.zeros((len(planes), n), dtype=t) for k, t in kinds.items()}
        self._check(self._lib.iblb_get_history_stats(self._h, *(_ptr(a) for a in arr.values())))
        return {m: {k: a[j] for k, a in arr.items()} for j, m in enumerate(planes)}

    def history_points(self) -> tuple[np.ndarray, np.ndarray]:
        """The fixed probes x [n], y [n] (iblb_get_history_points); an error when following tracers."""
        n = self.history_info()["n"]
        x, y = np.empty(n), np.empty(n)
        if n == 0:
            self._check(self._lib.iblb_get_history_points(self._h, None, None))
        self._check(self._lib.iblb_get_history_points(self._h, _ptr(x), _ptr(y)))
        return x, y

    # -- passive scalar ---------------------------------------------------------------------------
    def set_scalar(self, c0=None, g0=None, tau: float = 1.0, stride: int = 1,
                   walls=((L.SCALAR_WALL_NOFLUX, 0.0), (L.SCALAR_WALL_NOFLUX, 0.0))) -> None:
        """A concentration field that `step` advects with the fluid and diffuses on the device, D = (tau - 0.5)/3:
        `stride` substeps every `stride` iterations with the velocity of that moment (iblb_set_scalar).  c0:
        (ny, nx) concentrations, set to equilibrium at the current velocity; or g0: (5, ny, nx) populations as
        `scalar_populations` returns them (a restart).  walls: ((kind, value) below row 0, (kind, value) above
        the top row), kind L.SCALAR_WALL_NOFLUX or L.SCALAR_WALL_VALUE.  A lone slab only."""
        def arr(a, n):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != n:
                raise ValueError(f"expected {n} values, got {a.size}")
            return a
        c0, g0 = arr(c0, self.N), arr(g0, 5 * self.N)
        (k0, v0), (k1, v1) = walls
        cfg = L.Scalar(float(tau), int(stride), (C.c_int * 2)(int(k0), int(k1)),
                       (C.c_double * 2)(0.0 if v0 is None else float(v0), 0.0 if v1 is None else float(v1)))
        self._check(self._lib.iblb_set_scalar(self._h, C.byref(cfg), _ptr(c0), _ptr(g0)))

    def remove_scalar(self) -> None:
        """Remove the scalar: `step` is then exactly what it is without one."""
        self._check(self._lib.iblb_set_scalar(self._h, None, None, None))

    def scalar_info(self) -> dict:
        """{"tau", "stride", "walls": ((kind, value), (kind, value)), "updates"} of the scalar
        (iblb_scalar_info); stride == 0: none set."""
        cfg, n = L.Scalar(), C.c_longlong(0)
        self._check(self._lib.iblb_scalar_info(self._h, C.byref(cfg), C.byref(n)))
        return {"tau": cfg.tau, "stride": cfg.stride,
                "walls": tuple((cfg.wall_kind[k], cfg.wall_value[k]) for k in range(2)), "updates": n.value}

    def scalar(self, window=None) -> np.ndarray:
        """C on a strided window, (ny, nx) of the window (iblb_get_scalar); None: the whole lattice."""
        w = _window(window)
        shape = (self.ny, self.nx) if w is None else (max(w.ny, 0), max(w.nx, 0))
        out = np.empty(shape)
        self._check(self._lib.iblb_get_scalar(self._h, None if w is None else C.byref(w), _ptr(out)))
        return out

    def scalar_wall_flux(self) -> tuple[np.ndarray, np.ndarray]:
        """(bottom, top), [nx] each: the net amount of C that entered every column through the wall below row 0 /
        above the top row during the last substep (iblb_get_scalar_wall_flux); exact zeros at a no-flux wall, or
        the source's wall_flux there once `set_scalar_source` gave one.  The loss of `set_scalar_uptake` at a no-flux
        wall is not in it: `scalar_uptake()["last"]` is the full net."""
        bottom, top = np.empty(self.x_count), np.empty(self.x_count)
        self._check(self._lib.iblb_get_scalar_wall_flux(self._h, _ptr(bottom), _ptr(top)))
        return bottom, top

    def scalar_populations(self) -> np.ndarray:
        """The five post-stream populations, (5, ny, nx) (iblb_get_scalar_populations): what `set_scalar(g0=...)`
        takes."""
        g = np.empty((5, self.ny, self.x_count))
        self._check(self._lib.iblb_get_scalar_populations(self._h, _ptr(g)))
        return g

    def set_scalar_source(self, source=None, decay: float = 0.0, wall_flux=(None, None),
                          wall_value=(None, None)) -> None:
        """What enters and leaves the scalar from the next substep on (iblb_set_scalar_source).  source: (ny, nx),
        the amount of C added to a cell per substep; decay: the first-order loss per substep; wall_flux: (below
        row 0, above the top row), [nx] each or None, the amount entering a column per substep through a no-flux
        wall; wall_value: the same pair for the walls of kind L.SCALAR_WALL_VALUE, the wall value per column.
        Needs a scalar; replaces any previous source."""
        def arr(a, n):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != n:
                raise ValueError(f"expected {n} values, got {a.size}")
            return a
        source = arr(source, self.N)
        f0, f1 = (arr(a, self.x_count) for a in wall_flux)
        v0, v1 = (arr(a, self.x_count) for a in wall_value)
        src = L.ScalarSource(_addr(source), float(decay), (C.c_void_p * 2)(_addr(f0), _addr(f1)),
                             (C.c_void_p * 2)(_addr(v0), _addr(v1)))
        self._check(self._lib.iblb_set_scalar_source(self._h, C.byref(src)))

    def remove_scalar_source(self) -> None:
        """Remove the source: the scalar's substep is then exactly what it is without one."""
        self._check(self._lib.iblb_set_scalar_source(self._h, None))

    def scalar_source_info(self) -> dict:
        """{"decay", "present"} of the source (iblb_scalar_source_info); present: L.SCALAR_SOURCE_* bits, 0: none
        set."""
        k, m = C.c_double(0.0), C.c_uint(0)
        self._check(self._lib.iblb_scalar_source_info(self._h, C.byref(k), C.byref(m)))
        return {"decay": k.value, "present": m.value}

    def scalar_source(self) -> np.ndarray:
        """The bulk source as given, (ny, nx) (iblb_get_scalar_source); zeros where the source has none."""
        out = np.empty((self.ny, self.x_count))
        self._check(self._lib.iblb_get_scalar_source(self._h, _ptr(out)))
        return out

    def set_scalar_uptake(self, rate=(None, None)) -> None:
        """First-order uptake at the no-flux walls and per-column accumulators of what crossed each wall, from the
        next substep on (iblb_set_scalar_uptake).  rate: (below row 0, above the top row), [nx] each or None: the
        flux out of a column is rate * C at the wall, per substep; only at walls of kind L.SCALAR_WALL_NOFLUX.  With
        both None the uptake only accumulates.  Needs a scalar; replaces any previous uptake and zeroes its totals."""
        def arr(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != self.x_count:
                raise ValueError(f"expected {self.x_count} values, got {a.size}")
            return a
        r0, r1 = (arr(a) for a in rate)
        up = L.ScalarUptake((C.c_void_p * 2)(_addr(r0), _addr(r1)))
        self._check(self._lib.iblb_set_scalar_uptake(self._h, C.byref(up)))

    def remove_scalar_uptake(self) -> None:
        """Remove the uptake: the scalar's substep is then exactly what it is without one."""
        self._check(self._lib.iblb_set_scalar_uptake(self._h, None))

    def reset_scalar_uptake(self) -> None:
        """Zero the uptake's totals, last and substeps; the rates stay (iblb_reset_scalar_uptake)."""
        self._check(self._lib.iblb_reset_scalar_uptake(self._h))

    def scalar_uptake(self) -> dict:
        """{"total": (bottom, top), "last": (bottom, top), "substeps": n} (iblb_get_scalar_uptake), [nx] each: the
        net amount of C that entered every column through the wall below row 0 / above the top row since the set or
        the reset, and during the last substep (negative: absorbed)."""
        out = [np.empty(self.x_count) for _ in range(4)]
        n = C.c_longlong(0)
        self._check(self._lib.iblb_get_scalar_uptake(self._h, *(_ptr(a) for a in out), C.byref(n)))
        return {"total": (out[0], out[1]), "last": (out[2], out[3]), "substeps": n.value}

    def scalar_uptake_info(self) -> dict:
        """{"present", "substeps"} of the uptake (iblb_scalar_uptake_info); present: L.SCALAR_UPTAKE_* bits, 0: none
        set."""
        m, n = C.c_uint(0), C.c_longlong(0)
        self._check(self._lib.iblb_scalar_uptake_info(self._h, C.byref(m), C.byref(n)))
        return {"present": m.value, "substeps": n.value}

    def set_scalar_ends(self, kind=("value", "outflow"), value=(0.0, 0.0), profile=(None, None)) -> None:
        """Open ends in x for the scalar, from the next substep on (iblb_set_scalar_ends): nothing wraps from column
        nx - 1 to column 0 any more.  kind: (left of column 0, right of column nx - 1), each "noflux", "value" or
        "outflow" (or L.SCALAR_END_*); value: the uniform value of a "value" end; profile: [ny] each or None, the
        value per row in its place.  Per-row accumulators of what crossed each end start at zero (`scalar_ends`).
        Needs a scalar; replaces any previous ends.  The fluid stays periodic."""
        def arr(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != self.ny:
                raise ValueError(f"expected {self.ny} values, got {a.size}")
            return a
        kinds = [L.SCALAR_END_KINDS[k] if isinstance(k, str) else int(k) for k in kind]
        p0, p1 = (arr(a) for a in profile)
        ends = L.ScalarEnds((C.c_int * 2)(*kinds), (C.c_double * 2)(float(value[0]), float(value[1])),
                            (C.c_void_p * 2)(_addr(p0), _addr(p1)))
        self._check(self._lib.iblb_set_scalar_ends(self._h, C.byref(ends)))

    def remove_scalar_ends(self) -> None:
        """Remove the ends: the scalar is periodic in x again, its substep exactly what it is without them."""
        self._check(self._lib.iblb_set_scalar_ends(self._h, None))

    def reset_scalar_ends(self) -> None:
        """Zero the ends' totals, last and substeps; kinds and values stay (iblb_reset_scalar_ends)."""
        self._check(self._lib.iblb_reset_scalar_ends(self._h))

    def scalar_ends(self) -> dict:
        """{"total": (left, right), "last": (left, right), "substeps": n} (iblb_get_scalar_ends), [ny] each: the net
        amount of C that entered every row through the end left of column 0 / right of column nx - 1 since the set or
        the reset, and during the last substep (negative: it left)."""
        out = [np.empty(self.ny) for _ in range(4)]
        n = C.c_longlong(0)
        self._check(self._lib.iblb_get_scalar_ends(self._h, *(_ptr(a) for a in out), C.byref(n)))
        return {"total": (out[0], out[1]), "last": (out[2], out[3]), "substeps": n.value}

    def scalar_ends_info(self) -> dict:
        """{"kind", "value", "present", "substeps"} of the ends (iblb_scalar_ends_info); kind: a pair of
        L.SCALAR_END_*, value: as given; present: L.SCALAR_ENDS_* bits, 0: none set (kind and value are then None)."""
        k, v = (C.c_int * 2)(0, 0), (C.c_double * 2)(0.0, 0.0)
        m, n = C.c_uint(0), C.c_longlong(0)
        self._check(self._lib.iblb_scalar_ends_info(self._h, k, v, C.byref(m), C.byref(n)))
        return {"kind": tuple(k) if m.value else None, "value": tuple(v) if m.value else None, "present": m.value,
                "substeps": n.value}

    def set_scalar_gauges(self, stations=(), levels=()) -> None:
        """Transport gauges for the scalar, from the next substep on (iblb_set_scalar_gauges).  stations: columns x,
        strictly ascending in 0 .. nx - 1, each the link between column x and the column to its right; levels: rows
        y, strictly ascending in 0 .. ny - 2, each the link between row y and row y + 1.  Every substep adds the
        populations that cross those links to per-row / per-column totals, which start at zero (`scalar_gauges`).
        Needs a scalar; replaces any previous gauges.  No population changes."""
        st = np.ascontiguousarray(stations, dtype=np.intc).reshape(-1)
        lv = np.ascontiguousarray(levels, dtype=np.intc).reshape(-1)
        ga = L.ScalarGauges(st.size, _addr(st) if st.size else None, lv.size, _addr(lv) if lv.size else None)
        self._check(self._lib.iblb_set_scalar_gauges(self._h, C.byref(ga)))

    def remove_scalar_gauges(self) -> None:
        """Remove the gauges: the scalar's substep is then exactly what it is without them."""
        self._check(self._lib.iblb_set_scalar_gauges(self._h, None))

    def reset_scalar_gauges(self) -> None:
        """Zero the gauges' totals and substeps; the positions stay (iblb_reset_scalar_gauges)."""
        self._check(self._lib.iblb_reset_scalar_gauges(self._h))

    def scalar_gauges(self) -> dict:
        """{"right", "left", "up", "down", "substeps"} (iblb_get_scalar_gauges).  right, left: (n_stations, ny), the
        sums over the substeps of p_1 of the station's column and of p_2 of the column to its right, per row; up,
        down: (n_levels, nx), those of p_3 of the level's row and of p_4 of the row above, per column.  The net
        amount that crossed towards +x is right - left, towards +y up - down."""
        info = self.scalar_gauges_info()
        ns, nl = len(info["stations"]), len(info["levels"])
        right, left = np.empty((ns, self.ny)), np.empty((ns, self.ny))
        up, down = np.empty((nl, self.x_count)), np.empty((nl, self.x_count))
        n = C.c_longlong(0)
        self._check(self._lib.iblb_get_scalar_gauges(self._h, *(_ptr(a) for a in (right, left, up, down)), C.byref(n)))
        return {"right": right, "left": left, "up": up, "down": down, "substeps": n.value}

    def scalar_gauges_info(self) -> dict:
        """{"stations", "levels", "substeps"} of the gauges (iblb_scalar_gauges_info): the positions as given,
        tuples; none set: both empty and substeps 0."""
        ns, nl, n = C.c_int(0), C.c_int(0), C.c_longlong(0)
        self._check(self._lib.iblb_scalar_gauges_info(self._h, C.byref(ns), None, C.byref(nl), None, None))
        st, lv = np.zeros(ns.value, dtype=np.intc), np.zeros(nl.value, dtype=np.intc)
        self._check(self._lib.iblb_scalar_gauges_info(self._h, None, _ptr(st), None, _ptr(lv), C.byref(n)))
        return {"stations": tuple(int(v) for v in st), "levels": tuple(int(v) for v in lv), "substeps": n.value}

    @property
    def steps(self) -> int:
        n = C.c_longlong(0)
        self._check(self._lib.iblb_get_step(self._h, C.byref(n)))
        return n.value

    def count_nonfinite(self) -> int:
        """NaN / Inf stored populations of the current state (whole lattice; collective in an
        RCCL group)."""
        n = C.c_longlong(0)
        self._check(self._lib.iblb_count_nonfinite(self._h, C.byref(n)))
        return n.value

    # -- timing -----------------------------------------------------------------------------
    def set_profiling(self, on=True) -> None:
        """True / 1: events around every launch; 2: only the deep launches, by their own signals
        (include/iblb.h iblb_set_profiling); False / 0: off."""
        mode = 2 if (not isinstance(on, bool) and on == 2) else (1 if on else 0)
        self._check(self._lib.iblb_set_profiling(self._h, mode))

    def timing(self, reset: bool = False) -> dict:
        t = L.Timing()
        self._check(self._lib.iblb_get_timing_ex(self._h, C.byref(t), C.sizeof(t), 1 if reset else 0))
        return {k: getattr(t, k) for k, _ in L.Timing._fields_}

    def deep_force_build(self) -> int:
        """The collide build of the last deep launch (include/iblb.h iblb_deep_force_build): 1 the one
        for a body force along x only, 0 the general one, -1 no deep launch yet."""
        return int(self._lib.iblb_deep_force_build(self._h))

    @property
    def stream(self) -> int:
        s = C.c_void_p()
        self._check(self._lib.iblb_get_stream(self._h, C.byref(s)))
        return s.value or 0

    def synchronize(self) -> None:
        self._check(self._lib.iblb_synchronize(self._h))

    # -- checkpoint / restart -------------------------------------------------------------------
    def save_checkpoint(self, path, observers: int = 0) -> None:
        """The fluid (iblb_save_checkpoint); with observers, L.CKPT_* bits or L.OBSERVERS, also the scalar, the
        tracers and the averages that are asked for and set (iblb_save_checkpoint_ex).  `load_checkpoint` takes both."""
        if observers == 0:
            self._check(self._lib.iblb_save_checkpoint(self._h, os.fsencode(path)))
        else:
            self._check(self._lib.iblb_save_checkpoint_ex(self._h, os.fsencode(path), int(observers)))

    def load_checkpoint(self, path) -> None:
        self._check(self._lib.iblb_load_checkpoint(self._h, os.fsencode(path)))
        self.ns = int(np.fromfile(path, dtype=np.int64, count=9, offset=8)[7])

    # -- RCCL group ---------------------------------------------------------------------------
    def attach_rccl(self, unique_id: bytes, nranks: int, rank: int) -> None:
        if len(unique_id) != L.UNIQUE_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        self._check(self._lib.iblb_attach_rccl(self._h, unique_id, int(nranks), int(rank)))
        self.rank = int(rank)

    def set_wait_timeout(self, seconds: float) -> None:
        """Bound of the group's device-side waits (include/iblb.h iblb_set_wait_timeout; default
        600 s): a neighbour late by less changes nothing, a longer stall fails the call."""
        self._check(self._lib.iblb_set_wait_timeout(self._h, float(seconds)))

    def gather_macro(self, root: int = 0):
        """Whole-lattice rho [nx*ny], u [2*nx*ny] on rank `root` (None elsewhere); collective."""
        n = self.nx * self.ny
        rho, u = np.empty(n), np.empty(2 * n)
        self._check(self._lib.iblb_gather_macro(self._h, int(root), _ptr(rho), _ptr(u)))
        return (rho, u) if getattr(self, "rank", 0) == int(root) else (None, None)


def checkpoint_info(path, lib=None) -> dict:
    """{"step", "observers"} of a checkpoint file (iblb_checkpoint_info): the iteration it was saved at and the
    L.CKPT_* bits of the observers it holds.  Reads the file's header and framing only: no context, no device."""
    lib = lib or L.load()
    step, observers = C.c_longlong(0), C.c_uint(0)
    L.check(lib.iblb_checkpoint_info(os.fsencode(path), C.byref(step), C.byref(observers)), None, lib)
    return {"step": step.value, "observers": observers.value}


def rccl_unique_id(lib=None) -> bytes:
    lib = lib or L.load()
    buf = C.create_string_buffer(L.UNIQUE_ID_BYTES)
    L.check(lib.iblb_rccl_unique_id(buf), None, lib)
    return buf.raw


class LocalGroup:
    """Slabs of one process linked left to right (synchronous transport, for testing)."""

    def __init__(self, slabs: list[Lattice]):
        self.slabs = list(slabs)
        self._lib = self.slabs[0]._lib
        self._arr = (C.c_void_p * len(self.slabs))(*[s.handle for s in self.slabs])
        L.check(self._lib.iblb_link_local(self._arr, len(self.slabs)), self.slabs[0].handle, self._lib)

    def step(self, n: int = 1) -> None:
        rc = self._lib.iblb_group_step(self._arr, len(self.slabs), int(n))
        if rc != L.IBLB_OK:
            for s in self.slabs:
                msg = self._lib.iblb_last_error(s.handle)
                if msg:
                    raise L.IblbError(rc, msg.decode())
            L.check(rc, None, self._lib)

    def gather_macro(self) -> tuple[np.ndarray, np.ndarray]:
        """rho[N], u[2N] of the whole lattice in the reference layout."""
        ny = self.slabs[0].ny
        nx = self.slabs[0].nx
        rho = np.empty((ny, nx))
        u = np.empty((2, ny, nx))
        for s in self.slabs:
            r, uu = s.macro()
            rho[:, s.x_begin:s.x_begin + s.x_count] = r.reshape(ny, s.x_count)
            u[:, :, s.x_begin:s.x_begin + s.x_count] = uu.reshape(2, ny, s.x_count)
        return rho.ravel(), u.reshape(2, -1).ravel()

    def fields(self, names, window=None) -> dict:
        """Lattice.fields of every slab, joined along x: {name: array (ny, nx)} of the window.
        "vort" raises IBLB_ERR_UNSUPPORTED (a slab of a group does not compute it)."""
        parts = [s.fields(names, window) for s in self.slabs]
        return {n: np.concatenate([p[n] for p in parts], axis=1) for n in parts[0]}

    def reduce(self, names, window=None, rows=False, cols=False) -> dict:
        """Lattice.reduce of every slab merged by combine_stats: {name: Stats} of the whole window.
        "vort" raises IBLB_ERR_UNSUPPORTED (a slab of a group does not compute it)."""
        return combine_stats([s.reduce(names, window, rows, cols) for s in self.slabs])

    @property
    def flux(self) -> float:
        return math.fsum(s.flux for s in self.slabs)


def split_state(arr: np.ndarray, ncomp: int, nx: int, ny: int, x_begin: int, x_count: int) -> np.ndarray:
    """Slice a whole-lattice reference-layout field (SoA with ncomp blocks) to one slab."""
    a = np.asarray(arr).reshape(ncomp, ny, nx)[:, :, x_begin:x_begin + x_count]
    return np.ascontiguousarray(a).ravel()


def split_populations(f: np.ndarray, nx: int, ny: int, x_begin: int, x_count: int) -> np.ndarray:
    """Slice whole-lattice AoS populations f[9*j+i] to one slab."""
    a = np.asarray(f).reshape(ny, nx, 9)[:, x_begin:x_begin + x_count, :]
    return np.ascontiguousarray(a).ravel()
