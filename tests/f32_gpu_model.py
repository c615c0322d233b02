"""The GPU's f32 collide-stream iteration emulated in numpy (test infrastructure): every operation
of relax_cell<float, DEV = true> (csrc/iblb_device.h) in its order, each result rounded to float32,
fused multiply-adds evaluated in float64 and rounded once to float32 (the product of two float32
values is exact in float64, so only a sum that lands within 2^-29 of a float32 tie can round
differently from the hardware's fma), the collide constants folded in float32 as make_kbase /
make_kforce fold them.  Storage: deviations h = f - w_i, pull streaming with the reference's wall
rules (iblb_device.h:14-19).

Where tests/f32_model.py is an independent float32 restatement of the reference algorithm (the
precision's floor), this model is the GPU's own arithmetic on the CPU: its distance from the f64
oracle after n iterations says what the kernels' operation order costs in float32, without a GPU.
`variant` selects the order: "gpu" as the kernels compute it since round 4 — the odd
equilibrium part from the momentum rho u = m + F/2 itself and the rho-scaled constants as
c + (rho - 1) c, so the float32-rounded rho = 1 + (rho - 1) enters only through 1/rho; "r03" the
round-3 order (rho * constant, rho * (c.u)), which this emulation reproduces at the GPU's measured
round-3 errors (K1 128^2, 1000 iterations: rho - 1 1.8e-4, u_x 1.2e-6, u_y 8.9e-5).
`dtype=np.float64` runs the same operation order in double (what the order itself costs, without
float32); `mutate` seeds one named error into the collide (MUTATIONS), for the regime tests' power check.

F32GpuIBChannel adds the immersed-boundary iteration (csrc/ib_device.h, lbm_kernels.hip) in the
kernels' arithmetic: the force of an iteration from the stored post-collision state (the kernels' pull,
then Store<float>::to_f), node terms and the F_s fold in the reference's order and float rounding, the
spread in double, and the collide of a forced cell with constants folded from (float)(g + F).  Its
seeded errors are IB_MUTATIONS.
"""
from __future__ import annotations

import numpy as np

f32, f64 = np.float32, np.float64
C_S = 0.57735  # LatticeBoltzmann.cu:11
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])
WD = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
PA, PB = (1, 2, 5, 6), (3, 4, 7, 8)  # pairs (iblb_device.h pair_a / pair_b)


# Seeded errors (`mutate`) of the nonlinear and forcing terms, for the power check of the regime tests
# (tests/test_regimes.py::test_regimes_discriminate): what a kernel subtly wrong in that term computes.
MUTATIONS = {
    "M1": "the quadratic term (c.u)^2 / (2 cs^4) without rho (Qa = oqa)",
    "M2": "the -u^2 / (2 cs^2) term dropped (base = 0)",
    "M3": "the forcing's u.F part dropped",
    "M4": "the forcing's (c.u)(c.F) part dropped (hE = 0)",
    "M5": "kguo = 1 - 1/(2 tau2) instead of 1 - 1/(2 tau)",
    "M6": "c.u from the momentum m without F/2",
}


def fma(a, b, c):
    """Float32 operands: the fused result (see the module docstring).  Float64 operands (dtype=float64:
    the same operation order in double): product and sum rounded separately, 1e-16 away from fused."""
    t = np.result_type(a, b, c)
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(t)


def kconst(tau, tau2, gx, gy, dtype=np.float32, mutate=None):
    """make_kbase<float> / make_kforce<float> (iblb_device.h:167-210), contraction off; dtype=float64:
    make_kbase<double>."""
    assert mutate is None or mutate in MUTATIONS, mutate
    R = dtype  # the compute type: every constant below is folded in it
    op, om = R(1.0 / tau), R(1.0 / tau2)
    kk = R(1.0 - 1.0 / (2.0 * (tau2 if mutate == "M5" else tau)))
    ics2, ics4 = R(1.0 / (C_S * C_S)), R(1.0 / (C_S * C_S * C_S * C_S))
    a2 = R(1.0 / (2.0 * C_S * C_S * C_S * C_S))
    k = {"omp": R(1) - op, "opwr": op * R(4.0 / 9), "a1": R(1.0 / (2.0 * C_S * C_S))}
    for cl, w in ((0, R(1.0 / 9)), (1, R(1.0 / 36))):
        k[f"opw{cl}"] = op * w
        k[f"oqa{cl}"] = k[f"opw{cl}"] * a2
        k[f"omwi2{cl}"] = om * w * ics2
        kw = kk * w
        k[f"kwi4{cl}"] = kw * ics4
        k[f"kwi2{cl}"] = kw * ics2
        k[f"nck{cl}"] = -(ics2 * kw)
    k["hs"] = R(0.5) * k["omp"]
    k["hd"] = R(0.5) * (R(1) - om)
    Fx, Fy = R(gx), R(gy)
    k["Fx"], k["Fy"], k["hFx"], k["hFy"] = Fx, Fy, R(0.5) * Fx, R(0.5) * Fy
    cF = (Fx, Fy, Fx + Fy, Fy - Fx)
    for p in range(4):
        cl = 0 if p < 2 else 1
        k[f"hE{p}"] = cF[p] * k[f"kwi4{cl}"] if mutate != "M4" else R(0)
        k[f"gO{p}"] = cF[p] * k[f"kwi2{cl}"]
    return k


def relax(h, k, variant="gpu", mutate=None):
    """relax_cell<float, true> on arrays h[9, ...] of pulled deviations; returns h1.  The compute type is
    h's (float32, or float64 for the same order in double)."""
    R = h.dtype.type  # the compute type
    s = [h[PA[p]] + h[PB[p]] for p in range(4)]
    d = [h[PA[p]] - h[PB[p]] for p in range(4)]
    sm = h[0] + ((s[0] + s[1]) + (s[2] + s[3]))
    mx = d[0] + (d[2] - d[3])
    my = d[1] + (d[2] + d[3])
    rho = R(1) + sm
    inv = (f64(1) / rho.astype(f64)).astype(R)  # v_rcp_f32 + one Newton step
    jx, jy = mx + k["hFx"], my + k["hFy"]
    ux, uy = jx * inv, jy * inv
    usq = fma(uy, uy, ux * ux)
    uF = fma(uy, k["Fy"], ux * k["Fx"])
    base = (-usq) * k["a1"]
    if mutate == "M2":
        base = base * R(0)
    if mutate == "M3":
        uF = uF * R(0)
    cux, cuy = (mx * inv, my * inv) if mutate == "M6" else (ux, uy)
    rb = fma(rho, base, sm)
    out = np.empty_like(h)
    out[0] = fma(k["omp"], h[0], rb * k["opwr"])
    P, Qa, Rm = [], [], []
    for cl in (0, 1):
        P.append(fma(rb, k[f"opw{cl}"], uF * k[f"nck{cl}"]))
        if mutate == "M1":
            Qa.append(k[f"oqa{cl}"] + R(0) * sm)
        elif variant == "gpu":
            Qa.append(fma(sm, k[f"oqa{cl}"], k[f"oqa{cl}"]))
        else:
            Qa.append(rho * k[f"oqa{cl}"])
            Rm.append(rho * k[f"omwi2{cl}"])
    for p in range(4):
        cl = 0 if p < 2 else 1
        cu = (cux, cuy, cux + cuy, cuy - cux)[p]
        E = fma(cu, fma(Qa[cl], cu, k[f"hE{p}"]), P[cl])
        if variant == "gpu":  # rho (c.u) = c.(m + F/2): no rho, no 1/rho in the odd part
            cj = (jx, jy, jx + jy, jy - jx)[p]
            O = fma(k[f"omwi2{cl}"], cj, k[f"gO{p}"])
        else:
            O = fma(Rm[cl], cu, k[f"gO{p}"])
        A = fma(s[p], k["hs"], E)
        B = fma(d[p], k["hd"], O)
        out[PA[p]] = A + B
        out[PB[p]] = A - B
    return out


def pull(g):
    """f^t from the post-collision state g[9, ny, nx] (periodic x, bounce-back at y = 0, same-cell
    mirror at y = ny-1)."""
    f = np.empty_like(g)
    for i in range(9):
        src = np.roll(g[i], CX[i], axis=1)
        if CY[i] == 0:
            f[i] = src
        elif CY[i] == 1:
            f[i, 1:] = src[:-1]
        else:
            f[i, :-1] = src[1:]
    for k_, kk in ((2, 4), (5, 7), (6, 8)):
        f[k_, 0] = g[kk, 0]
    for k_, kk in ((4, 2), (8, 5), (7, 6)):
        f[k_, -1] = g[kk, -1]
    return f


class F32GpuChannel:
    """No-IB channel from rho, u (reference layout); the boot iteration in float64 (the GPU boots
    from the given double fields), then float32 iterations in the kernels' order."""

    def __init__(self, nx, ny, tau, tau2, rho, u, body_force, variant="gpu", dtype=np.float32, mutate=None):
        self.nx, self.ny, self.variant, self.mutate = nx, ny, variant, mutate
        self.k = kconst(tau, tau2, *body_force, dtype=dtype, mutate=mutate)
        rho = np.asarray(rho, f64).reshape(ny, nx)
        u = np.asarray(u, f64)
        ux, uy = u[:nx * ny].reshape(ny, nx), u[nx * ny:].reshape(ny, nx)
        gx, gy = body_force
        cs2 = C_S * C_S
        # boot: f^0 = feq(rho, u), collided with rho, u, the body force (equilibrium + Guo, TRT)
        usq = ux * ux + uy * uy
        feq = np.empty((9, ny, nx))
        Fi = np.empty((9, ny, nx))
        kg = 1.0 - 1.0 / (2.0 * tau)
        for i in range(9):
            cu = CX[i] * ux + CY[i] * uy
            feq[i] = rho * WD[i] * (1 + cu / cs2 + cu * cu / (2 * cs2 * cs2) - usq / (2 * cs2))
            vx = (CX[i] - ux) / cs2 + cu / (cs2 * cs2) * CX[i]
            vy = (CY[i] - uy) / cs2 + cu / (cs2 * cs2) * CY[i]
            Fi[i] = kg * WD[i] * (vx * gx + vy * gy)
        g = np.empty_like(feq)
        g[0] = feq[0]  # f = feq: the collision leaves f0, adds no F_0
        for a, b in zip(PA, PB):
            g[a] = feq[a] + Fi[a]
            g[b] = feq[b] + Fi[b]
        self.g = (g - WD[:, None, None]).astype(dtype)
        self.booted = False  # the boot collide above is the first iteration

    def step(self, n=1):
        for _ in range(n):
            if not self.booted:
                self.booted = True
                continue
            self.g = relax(pull(self.g), self.k, self.variant, self.mutate)

    def macro(self):
        """rho (= 1 + the deviation sum), u = (m + F/2)/rho, in float64 from the stored f32 state."""
        f = pull(self.g).astype(f64)
        dr = f.sum(axis=0)
        rho = 1.0 + dr
        mx = f[1] - f[3] + f[5] - f[6] - f[7] + f[8]
        my = f[2] - f[4] + f[5] + f[6] - f[7] - f[8]
        ux = (mx + 0.5 * float(self.k["Fx"])) / rho
        uy = (my + 0.5 * float(self.k["Fy"])) / rho
        return rho.ravel(), np.concatenate([ux.ravel(), uy.ravel()])


# ---- the immersed boundary -----------------------------------------------------------------------------
# Seeded one-term errors (`mutate` of F32GpuIBChannel) of the IB kernels, for the power check of the IB
# regime tests (tests/test_regimes.py::test_regimes_ib_discriminate).  A forced cell is one that a point's
# spread reached in this iteration.
IB_MUTATIONS = {
    "I1": "a forced cell's collide constants from the IB force alone ((float)(0 + F): the body force dropped)",
    "I2": "a forced cell's (c.u)(c.F) part (hE) from the body force alone",
    "I3": "node_term with rho taken as 1: 2 delta (u_s - m)",
    "I4": "nodes at x = -1 and x = XDIM read by a same-row periodic wrap instead of the flat index",
    "I5": "the F/2 of the velocity correction from the body force alone (j_x, j_y of a forced cell's collide, the reader's u)",
    "I6": "the spread at the points of the next iteration (off by one in a moving schedule)",
}


def d_delta(xs, ys, x, y):
    """d_delta (iblb_device.h:513-531; ImmersedBoundary.cu:21-81) on arrays: xs, ys float32, x, y integer.
    |x - xs| in float32, each 1-D factor in double rounded to float32, their product in float32."""
    def factor(xs, x):
        dx = np.abs(np.asarray(x).astype(f32) - xs)
        near, inside = dx <= f32(0.5), dx <= f32(1.5)
        dd = np.where(inside, dx, f32(0)).astype(f64)
        a = np.where(near, 0.33333, 0.16667)
        b = np.where(near, 1.0, 5.0 - 3.0 * dd)
        c = np.where(near, 1.0, -1.0)
        d = np.where(near, dd, np.where(inside, f32(1) - dx, f32(0)).astype(f64))
        return np.where(inside, a * (b + c * np.sqrt(-3.0 * d * d + 1.0)), 0.0).astype(f32)
    return factor(xs, x) * factor(ys, y)


def lifted_moments(g):
    """Store<T>::to_f of the pulled state ((double)h + w_i) and moments<double> of it (iblb_device.h:119-124):
    rho = f0 + ... + f8 in that order, m = sum c f in the reference's order."""
    f = pull(g).astype(f64) + WD[:, None, None]
    r = f[0]
    for i in range(1, 9):
        r = r + f[i]
    mx = ((((f[1] - f[3]) + f[5]) - f[6]) - f[7]) + f[8]
    my = ((((f[2] - f[4]) + f[5]) + f[6]) - f[7]) - f[8]
    return r, mx, my


class F32GpuIBChannel(F32GpuChannel):
    """The channel with Lagrangian points: `points` is (s, u_s, epsilon) (epsilon may be None) or
    points(it) for the points set before iteration `it` (0-based), as Simulation.set_lagrangian takes them.

    Iteration: collide-stream with the force of the previous iteration (the boot iteration with the body
    force), then the force of the new state from the points of this iteration: what ib_point_kernel /
    ib_ghost_kernel / ib_next_group evaluate from the stored post-collision state before the next collide,
    and the readers at the end of a call.  F_s and the float32 product F delta are float32 in both
    precisions, as in the kernels; dtype is the storage and collide type.

    spread_order: a permutation of the points, the order in which their terms reach a cell (the kernels:
    the arrival order of fp64 atomics).  perturb: a seed; every forced cell's cast force (float)(g + F) is
    moved by one ulp of the compute type up or down, seeded signs, in every iteration (the most a
    different arrival order can do to what the collide reads).  mutate: IB_MUTATIONS."""

    def __init__(self, nx, ny, tau, tau2, rho, u, body_force, points, dtype=np.float32, mutate=None,
                 spread_order=None, perturb=None):
        assert mutate is None or mutate in IB_MUTATIONS, mutate
        super().__init__(nx, ny, tau, tau2, rho, u, body_force, dtype=dtype)
        self.tau, self.tau2, self.dtype, self.ib_mutate = tau, tau2, dtype, mutate
        self.gx, self.gy = float(body_force[0]), float(body_force[1])
        self.points = points if callable(points) else (lambda it: points)
        self.order = None if spread_order is None else np.asarray(spread_order)
        self.rng = None if perturb is None else np.random.default_rng(perturb)
        self.it = 0
        self.fd = np.zeros((2, ny, nx))          # the dense IB force (without the body force)
        self.forced = np.zeros((ny, nx), bool)   # cells a spread term reached
        self.F_s = np.zeros(0, f32)

    def _points(self, it):
        s, us, eps = self.points(it)
        s, us = np.asarray(s, f32), np.asarray(us, f32)
        eps = np.ones(s.size // 2, np.int32) if eps is None else np.asarray(eps, np.int32)
        return s[0::2], s[1::2], us[0::2], us[1::2], eps

    @staticmethod
    def _nodes(xs, ys):
        """Node n of every point: (x, y) = (nearbyint(xs), nearbyint(ys)) + c_n, and its delta."""
        x = np.rint(xs.astype(f64)).astype(np.int64)[:, None] + CX[None, :]
        y = np.rint(ys.astype(f64)).astype(np.int64)[:, None] + CY[None, :]
        return x, y, d_delta(xs[:, None], ys[:, None], x, y)

    def _force(self, it):
        """node_term, the F_s fold and spread_node (ib_device.h) on the stored state."""
        nx, ny, m = self.nx, self.ny, self.ib_mutate
        xs, ys, usx, usy, eps = self._points(it)
        x, y, dl = self._nodes(xs, ys)
        j = y * nx + x  # flat index without wrap: column j % XDIM of row j / XDIM, left out beyond the lattice
        valid, xj, yj = (j >= 0) & (j < nx * ny), j % nx, j // nx
        if m == "I4":
            edge = (x == -1) | (x == nx)
            valid = np.where(edge, (y >= 0) & (y < ny), valid)
            xj, yj = np.where(edge, x % nx, xj), np.where(edge, y, yj)
        xj, yj = np.where(valid, xj, 0), np.where(valid, yj, 0)
        r, mx, my = (a[yj, xj] for a in lifted_moments(self.g))
        d2 = 2.0 * dl.astype(f64)
        if m == "I3":
            tx, ty = d2 * (usx.astype(f64)[:, None] - mx), d2 * (usy.astype(f64)[:, None] - my)
        else:
            tx = d2 * r * (usx.astype(f64)[:, None] - mx / r)
            ty = d2 * r * (usy.astype(f64)[:, None] - my / r)
        Fx, Fy = np.zeros(xs.size, f32), np.zeros(xs.size, f32)
        for n in range(9):  # fold_terms: node order, each partial sum rounded to float32
            Fx = np.where(valid[:, n], (Fx.astype(f64) + tx[:, n]).astype(f32), Fx)
            Fy = np.where(valid[:, n], (Fy.astype(f64) + ty[:, n]).astype(f32), Fy)
        self.F_s = np.stack([Fx, Fy], axis=1).ravel()
        if m == "I6":
            xs, ys, _, _, eps = self._points(it + 1)
            x, y, dl = self._nodes(xs, ys)
        # spread_node: clipped to the lattice (no periodic image), skipped where epsilon or delta is 0
        ok = (eps[:, None] != 0) & (x >= 0) & (x < nx) & (y >= 0) & (y < ny) & (dl != 0)
        e = eps.astype(f64)[:, None]
        px = (Fx[:, None] * dl).astype(f64) * 1.0 * e  # the float32 product, then double
        py = (Fy[:, None] * dl).astype(f64) * 1.0 * e
        o = np.arange(xs.size) if self.order is None else self.order
        ok_o = ok[o]
        self.fd = np.zeros((2, ny, nx))
        np.add.at(self.fd[0], (y[o][ok_o], x[o][ok_o]), px[o][ok_o])  # in the points' order, in double
        np.add.at(self.fd[1], (y[o][ok_o], x[o][ok_o]), py[o][ok_o])
        self.forced = np.zeros((ny, nx), bool)
        self.forced[y[ok], x[ok]] = True

    def _constants(self):
        """The collide constants per cell: make_kforce<R>(kb, (R)(gx + fx), (R)(gy + fy)); a cell without
        IB force gets (R)(gx + 0.0) = (R)gx, the body-force constants bit for bit."""
        R, m, forced = self.dtype, self.ib_mutate, self.forced
        Fx, Fy = (self.gx + self.fd[0]).astype(R), (self.gy + self.fd[1]).astype(R)
        if m == "I1":
            Fx, Fy = np.where(forced, self.fd[0].astype(R), Fx), np.where(forced, self.fd[1].astype(R), Fy)
        if self.rng is not None:
            sx, sy = self.rng.choice([-np.inf, np.inf], size=(2,) + forced.shape).astype(R)
            Fx, Fy = np.where(forced, np.nextafter(Fx, sx), Fx), np.where(forced, np.nextafter(Fy, sy), Fy)
        k = kconst(self.tau, self.tau2, Fx, Fy, dtype=R)
        if m == "I2":
            for p in range(4):
                k[f"hE{p}"] = np.where(forced, self.k[f"hE{p}"], k[f"hE{p}"])
        if m == "I5":
            k["hFx"], k["hFy"] = np.where(forced, self.k["hFx"], k["hFx"]), np.where(forced, self.k["hFy"], k["hFy"])
        return k

    def step(self, n=1):
        for _ in range(n):
            if self.booted:
                self.g = relax(pull(self.g), self._constants(), self.variant)
            self.booted = True  # (the boot collide of __init__ is the first iteration)
            self._force(self.it)
            self.it += 1

    def macro(self):
        """rho, u = (m + (F_dense + g)/2)/rho in float64 from the stored state (macro_out_kernel)."""
        r, mx, my = lifted_moments(self.g)
        fx, fy = (0.0, 0.0) if self.ib_mutate == "I5" else self.fd
        ux, uy = (mx + 0.5 * (fx + self.gx)) / r, (my + 0.5 * (fy + self.gy)) / r
        return r.ravel(), np.concatenate([ux.ravel(), uy.ravel()])

    def force(self):
        """The dense force with the body force, as iblb_get_force returns it."""
        return np.concatenate([(self.fd[0] + self.gx).ravel(), (self.fd[1] + self.gy).ravel()])

    def lagrangian_force(self):
        return self.F_s
