"""numpy restatement of the tracers' update rule under a motion model (include/iblb.h
iblb_set_tracer_model), on top of tracer_ref.sample: a field is an (ny, nx) array, field[y, x].

Every expression is written in the header's order with one numpy operation per arithmetic step, so that
each step is rounded once, as on the device; the hashes are uint64 arithmetic that wraps.  The results are
meant to be compared with `==`.
"""
import numpy as np

import tracer_ref as T

CLAMP, REFLECT, ABSORB = 0, 1, 2
ALIVE, AT_BOTTOM, AT_TOP = 0, 1, 2
WALLS = {"clamp": CLAMP, "reflect": REFLECT, "absorb": ABSORB}

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_S30, _S27, _S31, _S11 = np.uint64(30), np.uint64(27), np.uint64(31), np.uint64(11)


def mix(z):
    """The 64-bit finaliser of the header on a uint64 array (or scalar)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> _S30)
        z = z * _M1
        z = z ^ (z >> _S27)
        z = z * _M2
        z = z ^ (z >> _S31)
    return z


def raw(seed, p, m, k):
    """r_k of tracer(s) p at update m (before it: m updates done), k = 0 for x, 1 for y."""
    p = np.asarray(p, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = mix(np.uint64(seed) + GOLDEN * (p + np.uint64(1)))
        return mix(key + GOLDEN * np.uint64(2 * m + k + 1))


def xi(seed, p, m, k):
    """xi_k in [-1, 1): exact."""
    return (raw(seed, p, m, k) >> _S11).astype(np.float64) * 2.0 ** -52 - 1.0


def amplitude(diffusivity, stride):
    return float(np.sqrt(np.float64(6.0) * np.float64(diffusivity) * np.float64(stride)))


def step(su, sv, x, y, laps, status, hit, stride, m, t, shape, diffusivity=0.0, drift=(0.0, 0.0),
         walls=(CLAMP, CLAMP), seed=0):
    """One update given the sampled velocity (su, sv) at the tracers: steps 2 to 5 of the rule.  shape =
    (nx, ny).  Returns new (x, y, laps, status, hit, reflected), `reflected` the tracers a REFLECT wall folded
    back in this update; the inputs are left unchanged."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    laps = np.asarray(laps, dtype=np.int32)
    status = np.asarray(status, dtype=np.int32)
    hit = np.asarray(hit, dtype=np.int64)
    nx, ny = shape
    X, ytop, s = float(nx), float(ny - 1), float(stride)
    amp = amplitude(diffusivity, stride)
    p = np.arange(x.size, dtype=np.uint64)
    go = (status == ALIVE) & np.isfinite(su) & np.isfinite(sv)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xn = x + s * (su + float(drift[0]))
        yn = y + s * (sv + float(drift[1]))
        if amp != 0.0:
            xn = xn + amp * xi(seed, p, m, 0)
            yn = yn + amp * xi(seed, p, m, 1)
        low, high = yn < 0.0, yn > ytop
        kind = np.where(low, walls[0], walls[1])
        yw = np.where(low, 0.0, ytop)
        out = low | high
        absorb, reflect = out & (kind == ABSORB), out & (kind == REFLECT)
        lam = (yw - y) / (yn - y)
        xa = x + lam * (xn - x)
        yr = np.where(low, -yn, yw - (yn - yw))
        yr = np.where(yr < 0.0, 0.0, np.where(yr > ytop, ytop, yr))
        xn = np.where(absorb, xa, xn)
        yn = np.where(reflect, yr, np.where(out, yw, yn))
        up, down = xn >= X, xn < 0.0
        xw = np.where(up, xn - X, np.where(down, xn + X, xn))
        lw = laps + up.astype(np.int32) - down.astype(np.int32)
        moved = go & (xw >= 0.0) & (xw < X)  # else: more than one lattice length in one update
    dep = go & absorb
    st = np.where(dep, np.where(low, AT_BOTTOM, AT_TOP), status).astype(np.int32)
    ht = np.where(dep, np.int64(t), hit).astype(np.int64)
    return (np.where(moved, xw, x), np.where(go, yn, y), np.where(moved, lw, laps).astype(np.int32), st, ht,
            go & reflect)


def advect(ux, uy, x, y, laps, status, hit, stride, m, t, **model):
    """One update of the tracers in the velocity fields ux, uy ((ny, nx) arrays) held fixed."""
    ny, nx = np.asarray(ux).shape
    su, sv = T.sample(ux, x, y), T.sample(uy, x, y)
    return step(su, sv, x, y, laps, status, hit, stride, m, t, (nx, ny), **model)
