"""The reference-shaped kernels (include/iblb.h part 1, csrc/ref_kernels.hip) at every size, edge and entry point
of tests/dropin_cases.py against oracle/oracle.c.  The inputs are checked on the CPU by tests/test_dropin_cases.py:
the sparse sets reach no cell twice, so every comparison on them is `==`; 128 points or 128 contributions are not
enough on the sets that cross a workgroup; the flux column, the flux norm and the height of every
iblb_spread_ex case differ visibly from XDIM - 5, 192 and 192 rows.

Every device tensor, inputs included, has PAD trailing elements holding a sentinel, and every output is prefilled
with it.  PAD = 9 * 256: the 256 elements behind an output that a wrong tail guard of a 128-thread workgroup
writes, for the [9 N] arrays too, and a kernel whose guard is wrong still reads inside its allocations.  After
each call the trailing elements of every output must be unchanged (tails).

Bounds.  Everything is `==` but (a) the force and u of the dense sets and (b) the flux Q, where fp64 atomics add
in arrival order.  (a) d_delta is non-negative, so the oracle's spread fed |F_s| returns A_j = the sum of |term|
over the m_j points that reach cell j; two recursive sums of the same m_j terms in different orders differ by at
most (m_j - 1) 2^-53 A_j to first order, the bound on the force (0 where m_j = 1).  u = (sum_i c_i f_i +
force / 2) / rho: the same perturbation halved and divided by |rho_j|, plus one ulp of u for the two roundings
that follow.  (b) Q adds YDIM terms u_x / norm to its start value in any order: |Q_gpu - Q_oracle| <=
YDIM 2^-53 (|Q_start| + sum_y |u_x / norm|), the recursive-summation bound for YDIM + 1 terms; on the dense sets
the terms themselves differ by the bound on u, which is added over the column.  2^-53 is the only literal.

Measured on an MI355X (the tests print their figures): the dense sets' force and u equal the oracle's in every
cell (the terms are float products with 24-bit significands, and a dozen of them within 2^-15 of each other add
exactly in fp64 in any order); Q is off by at most 0.49 of its bound on the single calls (on YDIM = 4, where every
one of the 24 arrival orders stays inside the bound: tests/test_dropin_cases.py; <= 0.17 on 23 rows and more) and
by <= 0.11 of the summed bound in the chains.
"""
import functools

import numpy as np
import pytest

import dropin_cases as D

pytestmark = pytest.mark.gpu

PAD = 9 * 256
SENT = D.SENTINEL
TAU, TAU2 = D.TAU, D.TAU2


def _torch():
    import torch
    return torch


def _t(a):
    """A host array on the device, with the sentinel tail."""
    a = np.ascontiguousarray(a).ravel()
    return _torch().from_numpy(np.concatenate([a, np.full(PAD, SENT).astype(a.dtype)])).to("cuda")


def _out(n, dtype=None):
    """An output of n elements, prefilled with the sentinel like its tail."""
    torch = _torch()
    return torch.full((n + PAD,), SENT, dtype=dtype or torch.float64, device="cuda")


def _h(t, n):
    return t[:n].cpu().numpy()


def tails(**outs):
    """The PAD trailing elements of every output (name=(tensor, n)) still hold the sentinel."""
    for name, (t, n) in outs.items():
        bad = int((t[n:] != SENT).sum().item())
        assert bad == 0, f"{name}: {bad} of the {PAD} elements behind its end were written"


def same(got, ref, awkward=False):
    if not awkward:
        return np.array_equal(got, ref)
    fin = np.isfinite(ref)  # NaN payloads are not compared: the default NaN of x86 and of the GPU differ in sign
    return np.array_equal(got, ref, equal_nan=True) and np.array_equal(np.signbit(got[fin]), np.signbit(ref[fin]))


# ---- the four LBM kernels ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lbm_reference(X, Y, awkward):
    """Inputs and the oracle's outputs of the four kernels on a lattice, each kernel fed the oracle's own
    previous output.  The awkward state: the populations of dropin_cases.awkward_populations, and for the
    equilibrium their moments (rho = 0 with u = NaN, rho = inf, a subnormal rho)."""
    from oracle import oracle as O
    n = X * Y
    rho, u, force, f = D.lbm_state(X, Y)
    if awkward:
        f = D.awkward_populations(X, Y)
        rho, u = np.zeros(n), np.zeros(2 * n)
        O.macro(f, u, rho, X, Y)
    f0, F, f1, fs = np.zeros(9 * n), np.zeros(9 * n), np.zeros(9 * n), np.zeros(9 * n)
    us, rs, um, rm = np.zeros(2 * n), np.zeros(n), np.zeros(2 * n), np.zeros(n)
    O.equilibrium(u, rho, f0, force, F, X, Y, TAU)
    O.collision(f0, f, f1, F, TAU, TAU2, X, Y, 0)
    O.streaming(f1, fs, X, Y)
    O.macro(fs, us, rs, X, Y)
    O.macro(f, um, rm, X, Y)  # the moments of the populations themselves: on the awkward state inf / inf, 0 / 0
    return {"rho": rho, "u": u, "force": force, "f": f, "f0": f0, "F": F, "f1": f1, "fs": fs, "us": us, "rs": rs,
            "um": um, "rm": rm}


@pytest.mark.parametrize("awkward", [False, True], ids=["regular", "awkward"])
@pytest.mark.parametrize("shape", D.LBM_LATTICES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lbm_kernels(gpu, oracle, shape, awkward):
    """equilibrium, collision, streaming and macro on the tail-guard lattices, N = 2, 128, 129, 260 and 15: the
    oracle's bits (on the awkward state NaN where the oracle has NaN and the oracle's sign on every finite
    value), and nothing written behind f0, F, f1, f, u or rho."""
    from cuda_iblb_11_amd import kernels as K
    torch = _torch()
    X, Y = shape
    n = X * Y
    r = lbm_reference(X, Y, awkward)
    if awkward:
        assert np.isnan(r["f0"]).any() and np.isnan(r["f1"]).any() and np.isnan(r["um"]).any() and np.isinf(r["rm"]).any()
    df0, dF, df1, dfs, dus, drs = _out(9 * n), _out(9 * n), _out(9 * n), _out(9 * n), _out(2 * n), _out(n)
    dum, drm = _out(2 * n), _out(n)
    K.equilibrium(_t(r["u"]), _t(r["rho"]), df0, _t(r["force"]), dF, X, Y, TAU)
    K.collision(_t(r["f0"]), _t(r["f"]), df1, _t(r["F"]), TAU, TAU2, X, Y, 0)
    K.streaming(_t(r["f1"]), dfs, X, Y)
    K.macro(_t(r["fs"]), dus, drs, X, Y)
    K.macro(_t(r["f"]), dum, drm, X, Y)
    torch.cuda.synchronize()
    tails(f0=(df0, 9 * n), F=(dF, 9 * n), f1=(df1, 9 * n), f=(dfs, 9 * n), u=(dus, 2 * n), rho=(drs, n),
          u_of_f=(dum, 2 * n), rho_of_f=(drm, n))
    for name, t, m, key in [("equilibrium f0", df0, 9 * n, "f0"), ("equilibrium F", dF, 9 * n, "F"),
                            ("collision f1", df1, 9 * n, "f1"), ("streaming f", dfs, 9 * n, "fs"),
                            ("macro u", dus, 2 * n, "us"), ("macro rho", drs, n, "rs"),
                            ("macro u of f", dum, 2 * n, "um"), ("macro rho of f", drm, n, "rm")]:
        assert same(_h(t, m), r[key], awkward), (name, shape)


# ---- interpolate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", D.ALL_SETS, ids=D.ids(D.ALL_SETS))
def test_interpolate(gpu, oracle, ps):
    """F_s of every sparse, one-point and dense set equals the oracle's (a point's nine terms are added in one
    thread in the reference's order, so the dense sets are exact too): Ns on either side of 128, the flat-index
    rules on narrow and low lattices (x = -1 reads the previous row, x = XDIM the next, j outside [0, size) is
    skipped), half-integer coordinates."""
    from cuda_iblb_11_amd import kernels as K
    torch = _torch()
    ref = D.reference(ps.id)
    dFs = _out(2 * ps.ns, torch.float32)
    K.interpolate(_t(ref.rho), _t(ref.u), ps.ns, _t(ps.u_s), dFs, _t(ps.s), ps.X, ps.Y)
    torch.cuda.synchronize()
    tails(F_s=(dFs, 2 * ps.ns))
    got = _h(dFs, 2 * ps.ns)
    assert np.array_equal(got, ref.F_s), (ps.id, np.flatnonzero(got != ref.F_s)[:8])


def test_interpolate_no_points(gpu):
    """Ns == 0: IBLB_OK and a prefilled F_s is unchanged, with and without the point arrays."""
    from cuda_iblb_11_amd import kernels as K
    torch = _torch()
    X, Y = 37, 23
    rho, u, _ = D.field_state(X, Y)
    dFs = _out(16, torch.float32)
    K.interpolate(_t(rho), _t(u), 0, None, None, None, X, Y)
    K.interpolate(_t(rho), _t(u), 0, _t(np.zeros(16, dtype=np.float32)), dFs, _t(np.ones(16, dtype=np.float32)), X, Y)
    torch.cuda.synchronize()
    assert bool((dFs == SENT).all())


# ---- spread -----------------------------------------------------------------------------------------------------
def run_spread(K, ps, ref, **kw):
    """kernels.spread on a set from the oracle's F_s, force prefilled with the sentinel (the kernel clears it), Q
    started from Q0.  Returns force, u, Q on the host after the tail check."""
    torch = _torch()
    n = ps.X * ps.Y
    du, dforce, dQ = _t(ref.u), _out(2 * n), _t(np.array([D.Q0]))
    K.spread(_t(ref.rho), du, _t(ref.f), ps.ns, _t(ps.u_s), _t(ref.F_s), dforce, _t(ps.s), ps.X, dQ, _t(ps.eps), **kw)
    torch.cuda.synchronize()
    tails(force=(dforce, 2 * n), u=(du, 2 * n), Q=(dQ, 1))
    return _h(dforce, 2 * n), _h(du, 2 * n), float(_h(dQ, 1)[0])


def check_spread(ps, ref, force, u, Q):
    n = ps.X * ps.Y
    col, norm = D.flux_of(ps)
    if ps.kind == "dense":
        m1 = np.tile(np.maximum(ref.m - 1, 0), 2)
        b_force = m1 * D.U53 * ref.A
        b_u = 0.5 * b_force / np.abs(np.tile(ref.rho, 2)) + np.where(m1 > 0, np.spacing(np.abs(ref.u_out)), 0.0)
        e_force, e_u = np.abs(force - ref.force), np.abs(u - ref.u_out)
        on = b_force > 0
        print(ps.id, "cells off the oracle: force", int((e_force > 0).sum()), "u", int((e_u > 0).sum()),
              "worst error / bound", float(np.max(e_force[on] / b_force[on])))
        assert np.all(e_force <= b_force), (ps.id, np.flatnonzero(e_force > b_force)[:8])
        assert np.all(e_u <= b_u), (ps.id, np.flatnonzero(e_u > b_u)[:8])
        q_bound = ref.q_bound + float(np.sum(b_u[col:n:ps.X])) / abs(norm)
    else:
        assert np.array_equal(force, ref.force), (ps.id, np.flatnonzero(force != ref.force)[:8])
        assert np.array_equal(u, ref.u_out), (ps.id, np.flatnonzero(u != ref.u_out)[:8])
        q_bound = ref.q_bound
    print(ps.id, "Q", Q, "oracle", ref.Q[0], "error", abs(Q - ref.Q[0]), "bound", q_bound)
    assert abs(Q - ref.Q[0]) <= q_bound, (ps.id, Q, ref.Q[0], q_bound)


@pytest.mark.parametrize("ps", D.EX_SETS, ids=D.ids(D.EX_SETS))
def test_spread_ex(gpu, oracle, ps):
    """iblb_spread_ex with a YDIM (50, 23, 4), a flux column (0, XDIM - 1, XDIM // 3) and a flux norm (YDIM, 7.5)
    of its own, Q started from 0.125: force and u `==` on the sparse and one-point sets, within the per-cell bound
    of the module docstring on the dense sets; Q within the summation bound."""
    from cuda_iblb_11_amd import kernels as K
    ref = D.reference(ps.id)
    check_spread(ps, ref, *run_spread(K, ps, ref, **D.spread_kw(ps)))


def test_spread_192_rows_both_entries(gpu, oracle):
    """129 sparse points on (12, 192): iblb_spread (no YDIM, column or norm given) and iblb_spread_ex given 192,
    XDIM - 5 and 192 are both the oracle's, so equal to each other in force and u, as the header says."""
    from cuda_iblb_11_amd import kernels as K
    ps = D.SPARSE_192
    ref = D.reference(ps.id)
    a = run_spread(K, ps, ref)
    check_spread(ps, ref, *a)
    b = run_spread(K, ps, ref, YDIM=192, flux_column=ps.X - 5, flux_norm=192.0)
    check_spread(ps, ref, *b)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("shape", [(37, 23), (12, 192)], ids=["37x23-ex", "12x192"])
def test_spread_no_points(gpu, oracle, shape):
    """Ns == 0 with F_s, s and epsilon passed as None: force cleared, u the plain moment over rho, Q advanced."""
    from cuda_iblb_11_amd import kernels as K
    torch = _torch()
    X, Y = shape
    n = X * Y
    rho, u, f = D.field_state(X, Y)
    kw = {} if Y == 192 else {"YDIM": Y, "flux_column": X // 3, "flux_norm": 7.5}
    col, norm = (X - 5, 192.0) if Y == 192 else (X // 3, 7.5)
    none32, nonei = np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int32)
    fo, uo, Qo = np.full(2 * n, SENT), u.copy(), np.array([D.Q0])
    oracle.spread(rho, uo, f, 0, none32, none32, fo, none32, X, Qo, nonei, **({"YDIM": Y, **kw}))
    du, dforce, dQ = _t(u), _out(2 * n), _t(np.array([D.Q0]))
    K.spread(_t(rho), du, _t(f), 0, None, None, dforce, None, X, dQ, None, **kw)
    torch.cuda.synchronize()
    tails(force=(dforce, 2 * n), u=(du, 2 * n), Q=(dQ, 1))
    assert np.array_equal(_h(dforce, 2 * n), fo) and not fo.any()
    assert np.array_equal(_h(du, 2 * n), uo)
    bound = Y * D.U53 * (abs(D.Q0) + float(np.sum(np.abs(uo[col:n:X] / norm))))
    assert abs(float(_h(dQ, 1)[0]) - Qo[0]) <= bound


# ---- the six-launch chain ---------------------------------------------------------------------------------------
def run_chain(K, name, iters, stream=None, sync=None):
    """`iters` iterations of equilibrium, collision, streaming, macro, interpolate, spread on device arrays that
    start as oracle.Simulation's, the positions of iteration `it` taken from the table S[it] uploaded before the
    first launch.  Compares f, rho, u, force and F_s with `==` and Q within the summed bound at every snapshot
    of dropin_cases.chain_reference.  `stream` is passed to every kernel; `sync` waits for it before a read."""
    torch = _torch()
    c = D.CHAINS[name]
    X, Y, n, ns = c.X, c.Y, c.X * c.Y, c.ns
    snaps = D.chain_reference(name)
    rho, u, f, force = D.chain_init(c)
    kw = D.chain_spread_kw(c)
    drho, du, df, dforce = _t(rho), _t(u), _t(f), _t(force)
    df0, df1, dF, dQ = _out(9 * n), _out(9 * n), _out(9 * n), _t(np.zeros(1))
    if ns:
        S, u_s, eps = D.chain_points(c)
        dS = [_t(S[it]) for it in range(iters)]
        dus, deps, dFs = _t(u_s), _t(eps), _out(2 * ns, torch.float32)
    else:
        dS, dus, deps, dFs = [None] * iters, None, None, None
    sync = sync or torch.cuda.synchronize
    sync()
    torch.cuda.synchronize()  # the uploads above ran on the stream that was current
    seen = []
    for it in range(iters):
        K.equilibrium(du, drho, df0, dforce, dF, X, Y, TAU, stream=stream)
        K.collision(df0, df, df1, dF, TAU, TAU2, X, Y, it, stream=stream)
        K.streaming(df1, df, X, Y, stream=stream)
        K.macro(df, du, drho, X, Y, stream=stream)
        K.interpolate(drho, du, ns, dus, dFs, dS[it], X, Y, stream=stream)
        K.spread(drho, du, df, ns, dus, dFs, dforce, dS[it], X, dQ, deps, stream=stream, **kw)
        if c.body != (0.0, 0.0):  # as oracle_step adds it (oracle.c:415-418); chains with a body force run on
            dforce[:n] += c.body[0]  # the current stream only
            dforce[n:2 * n] += c.body[1]
        if it + 1 in snaps:
            sync()
            ref = snaps[it + 1]
            outs = {"f": (df, 9 * n), "rho": (drho, n), "u": (du, 2 * n), "force": (dforce, 2 * n), "f0": (df0, 9 * n),
                    "f1": (df1, 9 * n), "F": (dF, 9 * n), "Q": (dQ, 1)}
            if ns:
                outs["F_s"] = (dFs, 2 * ns)
            tails(**outs)
            for k in ("f", "rho", "u", "force") + (("F_s",) if ns else ()):
                got = _h(*outs[k])
                assert np.array_equal(got, ref[k]), (name, it + 1, k, np.flatnonzero(got != ref[k])[:8])
            q = float(_h(dQ, 1)[0])
            print(name, "iteration", it + 1, "Q", q, "oracle", ref["Q"], "error", abs(q - ref["Q"]), "bound", ref["q_bound"])
            assert abs(q - ref["Q"]) <= ref["q_bound"], (name, it + 1, q, ref["Q"], ref["q_bound"])
            seen.append(it + 1)
    sync()
    torch.cuda.synchronize()
    return seen


@pytest.mark.parametrize("name", list(D.CHAINS))
def test_chain(gpu, oracle, name):
    """25 iterations of the six launches, each kernel's output feeding the next (the corrected u into the next
    equilibrium, force cleared and rebuilt every iteration, Q accumulated throughout), after iterations 1, 2, 5
    and 25: (43, 3) without points and with a body force added to `force` on the host side; (48, 50) with 129
    sparse points that move by s += u_s every iteration, masked ones among them, flux column XDIM // 3 and norm
    YDIM; (12, 192) with the same kind of points through iblb_spread.  The references are oracle.Simulation
    (oracle_step) with points and the six oracle kernels in this order without (dropin_cases.six_launches)."""
    from cuda_iblb_11_amd import kernels as K
    assert run_chain(K, name, D.CHAIN_ITERS) == list(D.SNAP_AT)


@pytest.mark.parametrize("how", ["current", "explicit"])
def test_chain_on_a_side_stream(gpu, oracle, how):
    """The 129-point chain for 5 iterations on a stream that is not the NULL stream: entirely under
    `with torch.cuda.stream(side)`, and with stream=side passed to every kernel while the default stream is
    current (side.synchronize() before each read).  The same `==` as test_chain.  This pins that a non-NULL
    handle is accepted by every entry point and that the launches, the three of iblb_spread_ex included, keep
    their order on it; it is not a race detector."""
    from cuda_iblb_11_amd import kernels as K
    torch = _torch()
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0 and torch.cuda.current_stream().cuda_stream != side.cuda_stream
    torch.cuda.synchronize()
    if how == "current":
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream().cuda_stream == side.cuda_stream
            seen = run_chain(K, "moving", 5)
    else:
        seen = run_chain(K, "moving", 5, stream=side, sync=side.synchronize)
        assert torch.cuda.current_stream().cuda_stream != side.cuda_stream
    assert seen == [1, 2, 5]
