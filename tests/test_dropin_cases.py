"""The inputs of the drop-in kernel tests (tests/dropin_cases.py) checked on the CPU with the oracle alone, so
that tests/test_gpu_dropin.py can tell a wrong kernel from a right one:

* the sparse sets reach no cell twice (force, u, F_s are exact whatever the atomics' order), the dense sets reach
  some cell five times or more;
* a launch that covers only the first 128 points, or only the first 128 of the 9 Ns scatter contributions,
  changes F_s and force on every set large enough;
* on every lattice that is not 192 rows high, the flux column and the flux norm of the set differ in Q from
  XDIM - 5 and from 192, a point on row YDIM - 1 has a node row YDIM whose flat index a spread believing in 192
  rows would write (inside `force` and just past its end), and an interpolate node has size <= j < 192 XDIM;
* the sets on (3, 4) and (37, 23) reach interpolate's flat-index rule: a periodic wrap in x and a skip of the
  nodes outside in x both give another F_s;
* the oracle's two forms of the spread agree bit for bit on the sparse sets;
* the six oracle kernels in the drop-in order are oracle_step, and the chains keep their 4-cell spacing;
* every argument refusal of csrc/ref_kernels.hip, which returns before any launch and needs no device.
"""
import ctypes as C

import numpy as np
import pytest

import dropin_cases as D
from cuda_iblb_11_amd import _lib as L

NOT_192 = [p for p in D.ALL_SETS if p.Y != 192]


# ---- the point sets ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", D.ALL_SETS, ids=D.ids(D.ALL_SETS))
def test_reach(ps):
    m = D.reach(ps)
    print(ps.id, "cells reached", int((m > 0).sum()), "worst", int(m.max()))
    if ps.kind == "dense":
        assert m.max() >= 5
    else:
        assert m.max() <= 1
    assert ps.s.dtype == np.float32 and ps.s.size == 2 * ps.ns and ps.eps.size == ps.ns
    if ps.column is not None:
        assert ps.column != ps.X - 5 and ps.norm != 192.0 and 0 <= ps.column < ps.X


def test_set_shapes():
    """What the sets are meant to hold is there."""
    assert [p.ns for p in D.SPARSE_48] == [1, 14, 15, 127, 128, 129]
    assert {(p.column, p.norm) for p in D.EX_SETS if (p.X, p.Y) == (48, 50)} >= {(0, 50.0), (47, 7.5), (16, 50.0)}
    assert {p.column for p in D.EX_SETS if (p.X, p.Y) == (37, 23)} == {0, 36, 12}
    assert {p.norm for p in D.EX_SETS if (p.X, p.Y) == (37, 23)} == {23.0, 7.5}
    assert {p.Y for p in D.EX_SETS} == {50, 23, 4}
    ps = D.SPARSE_37
    x0, y0 = np.rint(ps.s[0::2]).astype(int), np.rint(ps.s[1::2]).astype(int)
    at = set(zip(x0, y0))
    assert (0, 0) in at and (36, 22) in at and (0, 22) in at and (36, 0) in at
    assert (y0 == 0).sum() == 10 and (y0 == 22).sum() == 10 and (x0 == 0).sum() == 6 and (x0 == 36).sum() == 6
    fr = ps.s.astype(np.float64) % 1
    assert (fr == 0.5).sum() == 4 and ((fr > 0.4999) & (fr < 0.5)).sum() == 4 and ((fr > 0.5) & (fr < 0.5001)).sum() == 4
    assert (ps.eps == 0).sum() == 12 and D.SPARSE_48[-1].eps[128] == 1
    assert sorted(int(np.rint(p.s[0])) for p in D.ONE_POINT) == [0, 0, 1, 2]
    for p in D.DENSE:
        y0 = np.rint(p.s[1::2])
        assert y0.min() == 0 and y0.max() == p.Y - 1 and p.s[0::2].min() < 0.5 and p.s[0::2].max() > p.X - 1.5


@pytest.mark.parametrize("ps", [p for p in D.ALL_SETS if p.ns > 128], ids=lambda p: p.id)
def test_first_128_points_are_not_enough(oracle, ps):
    """interpolate_k launched with one workgroup, or spread over the first 128 points only."""
    ref = D.reference(ps.id)
    for prefill in (0.0, D.SENTINEL):
        cut = np.full(2 * ps.ns, prefill, dtype=np.float32)
        oracle.interpolate(ref.rho, ref.u, 128, ps.u_s, cut, ps.s, ps.X, ps.Y)
        assert np.array_equal(cut[:256], ref.F_s[:256]) and np.all(cut[256:] != ref.F_s[256:])
    n = ps.X * ps.Y
    force, u, Q = np.zeros(2 * n), ref.u.copy(), np.array([D.Q0])
    oracle.spread(ref.rho, u, ref.f, 128, ps.u_s, ref.F_s, force, ps.s, ps.X, Q, ps.eps, **D.spread_kw(ps))
    assert not np.array_equal(force, ref.force) and not np.array_equal(u, ref.u_out)


@pytest.mark.parametrize("ps", [p for p in D.ALL_SETS if 9 * p.ns > 128], ids=lambda p: p.id)
def test_first_128_contributions_are_not_enough(oracle, ps):
    """spread_scatter_k launched with one workgroup covers 128 of the 9 Ns contributions, launched with nblk(Ns)
    workgroups 128 ceil(Ns / 128) of them: the scatter in numpy, point after point, equals the oracle's force in
    full (on the dense sets too: a cell's terms arrive in point order) and differs when cut at either count.
    Ns = 15 is the smallest set it shows on (contributions 128 ... 134 are point 14's)."""
    ref = D.reference(ps.id)
    assert np.array_equal(D.np_spread_force(ps, ref.F_s), ref.force)
    for limit in {128, 128 * ((ps.ns + 127) // 128)}:
        assert not np.array_equal(D.np_spread_force(ps, ref.F_s, limit=limit), ref.force), limit


def test_14_points_fit_one_workgroup():
    assert 9 * 14 < 128 < 9 * 15


@pytest.mark.parametrize("ps", NOT_192, ids=D.ids(NOT_192))
def test_flux_arguments_show(oracle, ps):
    ref = D.reference(ps.id)
    n = ps.X * ps.Y

    def q(column, norm):
        force, u, Q = np.zeros(2 * n), ref.u.copy(), np.array([D.Q0])
        oracle.spread(ref.rho, u, ref.f, ps.ns, ps.u_s, ref.F_s, force, ps.s, ps.X, Q, ps.eps, YDIM=ps.Y,
                      flux_column=column, flux_norm=norm)
        assert np.array_equal(force, ref.force) and np.array_equal(u, ref.u_out)
        return Q[0]

    assert q(ps.column, ps.norm) == ref.Q[0] != D.Q0
    assert q(ps.X - 5, ps.norm) != ref.Q[0]
    assert q(ps.column, 192.0) != ref.Q[0]
    assert 2 * ref.q_bound < min(abs(ref.Q[0] - q(ps.column, 192.0)), abs(ref.Q[0] - q(ps.X - 5, ps.norm)))


@pytest.mark.parametrize("ps", D.ONE_POINT, ids=D.ids(D.ONE_POINT))
def test_flux_bound_holds_for_every_arrival_order(oracle, ps):
    """On YDIM = 4 the flux bound is at its tightest; each of the 24 orders in which the atomics can add the
    column's terms to Q0 stays inside it."""
    import itertools
    ref = D.reference(ps.id)
    terms = [float(t) for t in ref.u_out[ps.column:ps.X * ps.Y:ps.X] / ps.norm]
    assert len(terms) == ps.Y == 4
    worst = 0.0
    for order in itertools.permutations(terms):
        q = D.Q0
        for t in order:
            q += t
        worst = max(worst, abs(q - ref.Q[0]))
    print(ps.id, "worst order / bound", worst / ref.q_bound)
    assert worst <= ref.q_bound


@pytest.mark.parametrize("ps", [D.SPARSE_37, D.SPARSE_48[-1], D.ONE_POINT[2]] + D.DENSE, ids=lambda p: p.id)
def test_a_spread_believing_in_192_rows_writes_row_ydim(oracle, ps):
    """Points on row YDIM - 1: their node row YDIM passes a clip at 192, and its flat index lies inside `force`
    (the y component's row 0 for the x component) or in the 256 elements past its end (the y component), with a
    non-zero term to add."""
    ref = D.reference(ps.id)
    size = ps.X * ps.Y
    hits = 0
    for k, n, x, y in D.nodes(ps):
        if y == ps.Y and 0 <= x < ps.X:
            assert y < 192
            j = y * ps.X + x
            assert size <= j < 2 * size                             # the x component lands in the y component
            assert 2 * size <= size + j < 2 * size + 256           # the y component lands past the end
            d = oracle.d_delta(float(ps.s[2 * k]), float(ps.s[2 * k + 1]), x, y)
            hits += bool(d != 0 and ps.eps[k] != 0 and ref.F_s[2 * k] != 0 and ref.F_s[2 * k + 1] != 0)
    assert hits >= 1
    # ... and some interpolate node has size <= j < 192 XDIM
    assert any(size <= y * ps.X + x < 192 * ps.X for _, _, x, y in D.nodes(ps))


@pytest.mark.parametrize("ps", [D.SPARSE_37] + D.ONE_POINT + D.DENSE, ids=lambda p: p.id)
def test_flat_index_rule_is_reached(oracle, ps):
    ref = D.reference(ps.id)
    assert np.array_equal(D.np_interpolate(ps, ref.rho, ref.u, "flat"), ref.F_s)
    if ps.id == D.ONE_POINT[1].id:  # x0 = 1 on three columns: no node outside in x
        return
    for rule in ("wrap", "skip"):
        assert not np.array_equal(D.np_interpolate(ps, ref.rho, ref.u, rule), ref.F_s), rule


@pytest.mark.parametrize("ps", D.SPARSE + D.ONE_POINT + [D.SPARSE_192], ids=lambda p: p.id)
def test_both_forms_of_the_oracle_spread_agree(oracle, ps):
    ref = D.reference(ps.id)
    n = ps.X * ps.Y
    force, u, Q = np.full(2 * n, D.SENTINEL), ref.u.copy(), np.array([D.Q0])
    oracle.spread(ref.rho, u, ref.f, ps.ns, ps.u_s, ref.F_s, force, ps.s, ps.X, Q, ps.eps, point_centric=True,
                  **D.spread_kw(ps))
    assert np.array_equal(force, ref.force) and np.array_equal(u, ref.u_out) and Q[0] == ref.Q[0]
    assert np.any(ref.force != 0) and np.any(ref.F_s != 0)


# ---- the LBM states ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", D.LBM_LATTICES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_awkward_state(oracle, shape):
    X, Y = shape
    n = X * Y
    f = D.awkward_populations(X, Y)
    sub, zero, (ci, pi), (cz, pz) = D.awkward_cells(n)
    assert np.all(f[9 * zero:9 * zero + 9] == 0) and f[9 * ci + pi] == np.inf
    assert f[9 * cz + pz] == 0 and np.signbit(f[9 * cz + pz])
    if n >= 4:
        assert len({sub, zero, ci, cz}) == 4 or (cz == ci and pz != pi)
        cell = f[9 * sub:9 * sub + 9]
        assert np.all(cell > 0) and np.all(cell < np.finfo(np.float64).tiny)
    u, rho = np.zeros(2 * n), np.zeros(n)
    with np.errstate(all="ignore"):
        oracle.macro(f, u, rho, X, Y)
    assert rho[zero] == 0 and np.isnan(u[zero]) and rho[ci] == np.inf and np.isnan(u[ci])
    if n >= 4:
        assert 0 < rho[sub] < np.finfo(np.float64).tiny and np.isfinite(u[sub])
    assert {128, 129} <= {a * b for a, b in D.LBM_LATTICES} and (1, 2) in D.LBM_LATTICES


# ---- the chain --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["moving", "rows192"])
def test_chain_points_keep_their_spacing(name):
    c = D.CHAINS[name]
    S, u_s, eps = D.chain_points(c)
    first = D.nodes(D.PointSet("", "sparse", c.X, c.Y, c.ns, S[0], u_s, eps, None, None))
    for it in range(D.CHAIN_ITERS):
        ps = D.PointSet("", "sparse", c.X, c.Y, c.ns, S[it], u_s, eps, None, None)
        assert D.reach(ps).max() == 1 and D.nodes(ps) == first, it
    assert not np.array_equal(S[-1], S[0]) and (eps == 0).sum() >= 20 and c.ns == 129
    assert float(np.max(np.abs(S[-1] - S[0]))) <= D.CHAIN_ITERS * D.CHAIN_SPEED


@pytest.mark.parametrize("name", list(D.CHAINS))
def test_chain_reference(oracle, name):
    """The references stay finite, the force is rebuilt every iteration and the flux bound stays far below
    the flux."""
    snaps = D.chain_reference(name)
    assert sorted(snaps) == list(D.SNAP_AT)
    last = snaps[D.CHAIN_ITERS]
    for k in ("f", "rho", "u", "force", "F_s"):
        assert np.all(np.isfinite(last[k])), k
    print(name, "max|u|", float(np.max(np.abs(last["u"]))), "Q", last["Q"], "bound", last["q_bound"])
    assert float(np.max(np.abs(last["u"]))) <= 0.1
    assert not np.array_equal(snaps[1]["f"], snaps[2]["f"]) and 0 < last["q_bound"] < 1e-9 * abs(last["Q"])
    if D.CHAINS[name].ns:
        assert not np.array_equal(snaps[1]["force"], snaps[2]["force"]) and np.any(last["F_s"] != 0)
        # a force that is not cleared accumulates: twice the force of one iteration is not what iteration 2 holds
        assert not np.array_equal(snaps[1]["force"] + snaps[2]["force"], snaps[2]["force"])


@pytest.mark.parametrize("name", ["moving", "rows192"])
def test_six_launches_are_oracle_step(oracle, name):
    """dropin_cases.six_launches, the reference of the chain without points, is oracle_step bit for bit where
    both are defined (points, no body force): 5 iterations against chain_reference (oracle.Simulation)."""
    c = D.CHAINS[name]
    S, u_s, eps = D.chain_points(c)
    st = D.new_chain_state(c)
    snaps = D.chain_reference(name)
    for it in range(5):
        D.six_launches(oracle, c, st, (S[it], u_s, eps))
        if it + 1 in snaps:
            for k in ("f", "rho", "u", "force", "F_s"):
                assert np.array_equal(st[k], snaps[it + 1][k]), (it, k)
            assert st["Q"][0] == snaps[it + 1]["Q"]


# ---- argument refusals (csrc/ref_kernels.hip): before any launch, no device needed -----------------------------
P = 0x1000  # a dummy non-null pointer: never dereferenced, every case below is refused (or has nothing to do)
TAUS = (D.TAU, D.TAU2)

# name -> (arguments that would launch, positions of the pointers that must not be NULL, (XDIM, YDIM) positions)
ENTRY = {
    "iblb_equilibrium": ([P, P, P, P, P, 4, 4, TAUS[0], None], [0, 1, 2, 3, 4], (5, 6)),
    "iblb_collision": ([P, P + 8, P + 16, P, TAUS[0], TAUS[1], 4, 4, 0, None], [0, 1, 2, 3], (6, 7)),
    "iblb_streaming": ([P, P + 8, 4, 4, None], [0, 1], (2, 3)),
    "iblb_macro": ([P, P, P, 4, 4, None], [0, 1, 2], (3, 4)),
    "iblb_interpolate": ([P, P, 1, P, P, P, 4, 4, None], [0, 1, 3, 4, 5], (6, 7)),
    # u_s (position 4) is unused by the reference's spread and by this one: NULL is accepted there
    "iblb_spread_ex": ([P, P, P, 1, P, P, P, P, 4, 4, P, P, 1, 4.0, None], [0, 1, 2, 5, 6, 7, 10, 11], (8, 9)),
    "iblb_spread": ([P, P, P, 1, P, P, P, P, 4, P, P, None], [0, 1, 2, 5, 6, 7, 9, 10], (8, None)),
    "iblb_delta": ([1, P, P, P, P, P, None], [1, 2, 3, 4, 5], None),
}


def _refusals():
    out = []
    for name, (args, ptrs, grid) in ENTRY.items():
        for p in ptrs:
            out.append((f"{name}-null{p}", name, {p: None}))
        if grid:
            out.append((f"{name}-xdim0", name, {grid[0]: 0}))
            out.append((f"{name}-xdim-3", name, {grid[0]: -3}))
            if grid[1] is not None:
                out.append((f"{name}-ydim1", name, {grid[1]: 1}))
                out.append((f"{name}-ydim0", name, {grid[1]: 0}))
    out.append(("iblb_streaming-f1-is-f", "iblb_streaming", {1: P}))
    for name in ("iblb_interpolate", "iblb_spread_ex", "iblb_spread"):
        out.append((f"{name}-ns-1", name, {2 if name == "iblb_interpolate" else 3: -1}))
    out.append(("iblb_spread_ex-norm0", "iblb_spread_ex", {13: 0.0}))
    out.append(("iblb_spread_ex-norm-0", "iblb_spread_ex", {13: -0.0}))
    out.append(("iblb_delta-n-1", "iblb_delta", {0: -1}))
    return out


@pytest.mark.parametrize("case", _refusals(), ids=[c[0] for c in _refusals()])
def test_refusals(case):
    _, name, change = case
    args = list(ENTRY[name][0])
    assert len(change) == 1  # exactly one offending argument: nothing is ever launched
    for k, v in change.items():
        assert args[k] != v
        args[k] = v
    assert getattr(L.load(), name)(*args) == L.IBLB_ERR_ARG


def test_entry_table_matches_the_signatures():
    """ENTRY lists each entry point with the argument count of its ctypes signature."""
    for name, (args, ptrs, grid) in ENTRY.items():
        sig = L._SIGS[name][0]
        assert len(args) == len(sig), name
        for p in ptrs:
            assert sig[p] is C.c_void_p, (name, p)


def test_nothing_to_do_is_ok():
    lib = L.load()
    assert lib.iblb_interpolate(P, P, 0, None, None, None, 4, 4, None) == L.IBLB_OK
    assert lib.iblb_interpolate(None, None, 0, None, None, None, 4, 4, None) == L.IBLB_OK
    assert lib.iblb_delta(0, None, None, None, None, None, None) == L.IBLB_OK
    assert lib.iblb_delta(0, P, P, P, P, P, None) == L.IBLB_OK
