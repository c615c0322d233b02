"""tests/scalar_matrix.py, the cases of the passive scalar's build matrix, pinned on the CPU with the numpy restatements
alone, so that tests/test_gpu_scalar_matrix.py cannot pass vacuously: in every case every switched-on feature changes
what the restatement returns, every slot of a pair (the two walls, the two ends, the two rates) shows when it is
swapped, and the sets the GPU file runs cover every combination under every wall pair, all nine pairs of end kinds with
gauges and without, and every end kind at each side below a _VALUE wall.

A seeded synthetic velocity with |u| <= 0.05, tau 0.8, two events of stride 3: six substeps.  No condition here depends
on a device; if one fails, the case's seed or magnitudes are wrong, not the condition.
"""
import itertools

import numpy as np
import pytest

import scalar_matrix as M
import scalar_ref as S
import scalar_source_ref as Q
import scalar_uptake_ref as U
import scalar_ends_ref as E
import scalar_gauges_ref as G

TAU = 0.8
STRIDE = 3
EVENTS = 2

_STATE = {}


def synthetic(nx, ny):
    """(g0, ux, uy): the equilibrium of a seeded C in [0, 1) with a step across the channel's middle at a seeded
    velocity, |u| <= 0.05 (computed once per size)."""
    if (nx, ny) not in _STATE:
        rng = np.random.default_rng(nx * 1009 + ny)
        c0 = rng.uniform(0.0, 0.5, (ny, nx))
        c0[: ny // 2] += 0.5
        ux, uy = rng.uniform(-0.05, 0.05, (2, ny, nx))
        g0 = S.equilibrium(c0, ux, uy)
        for a in (g0, ux, uy):
            a.setflags(write=False)
        _STATE[(nx, ny)] = (g0, ux, uy)
    return _STATE[(nx, ny)]


class Run:
    """Two events of one setting: the populations and every family of sums the setting has."""

    def __init__(self, nx, ny, ends, up, src, gauges, walls):
        g, ux, uy = synthetic(nx, ny)
        sums = None if gauges is None else G.Sums(gauges, nx, ny)
        es = None if ends is None else E.Sums(ny)
        us = None if up is None else U.Sums(nx)
        for _ in range(EVENTS):
            g, sums, es, us = G.event(g, ux, uy, TAU, STRIDE, gauges, sums, ends, es, up, us, src, walls)
        self.g, self.sums, self.es, self.us = g, sums, es, us

    def arrays(self):
        out = {"g": self.g}
        if self.sums is not None:
            out.update({n: getattr(self.sums, n) for n in ("right", "left", "up", "down")})
        for name, s in (("ends", self.es), ("uptake", self.us)):
            if s is not None:
                out[name + " total"], out[name + " last"] = s.total, s.last
        return out

    def differs_from(self, other):
        """The populations differ, or a family of sums that both runs hold does."""
        a, b = self.arrays(), other.arrays()
        return any(not np.array_equal(a[n], b[n]) for n in a if n in b)


def mirrored_walls(up, src, walls):
    """Everything the case holds per wall with its two slots swapped: the kinds and values, the source's wall arrays
    and the uptake's rates (each array stays with its wall, so the rules of include/iblb.h still hold)."""
    src2 = None if src is None else Q.Source(src.source, src.decay, src.wall_flux[::-1], src.wall_value[::-1])
    up2 = None if up is None else U.Uptake(up.rate[::-1])
    return up2, src2, (walls[1], walls[0])


@pytest.mark.parametrize("nx,ny,ci,walls_name", M.matrix(),
                         ids=[M.case_id(*c) for c in M.matrix()])
def test_every_feature_and_every_slot_shows(nx, ny, ci, walls_name):
    combo = M.COMBOS[ci]
    ends, up, src, gauges, walls = M.case(nx, ny, combo, walls_name)
    assert [v is not None for v in (src, up, ends, gauges)] == list(combo)
    base = Run(nx, ny, ends, up, src, gauges, walls)
    for name, a in base.arrays().items():
        assert np.all(np.isfinite(a)), name
    for s in (base.sums, base.es, base.us):
        assert s is None or s.substeps == STRIDE * EVENTS == 6

    # every switched-on feature is visible
    if src is not None:
        assert not np.array_equal(Run(nx, ny, ends, up, None, gauges, walls).g, base.g), "the source"
    if ends is not None:
        same = np.array_equal(Run(nx, ny, None, up, src, gauges, walls).g, base.g)
        # one column with outflow at both ends: g_1'(0) = p_1(0) and g_2'(0) = p_2(0) by the ends' rule, which is
        # what the wrap onto the same column gives: the populations are the periodic ones by the rule itself, and the
        # ends show in their totals alone (net = p_1 - p_2 and its opposite)
        assert same == (nx == 1 and ends.kind == (E.OUTFLOW, E.OUTFLOW)), "the ends"
        if same:
            assert np.all(base.es.total != 0.0) and np.all(base.es.last != 0.0), "the ends' totals"
    if up is not None:
        if any(r is not None for r in up.rate):
            assert not np.array_equal(Run(nx, ny, ends, None, src, gauges, walls).g, base.g), "the uptake"
        for k in range(2):  # what crossed a _VALUE wall is accumulated whether or not the uptake has a rate
            if walls[k][0] == S.VALUE:
                assert np.all(base.us.total[k] != 0.0) and np.all(base.us.last[k] != 0.0), ("the uptake's totals", k)
        if all(r is None for r in up.rate):
            assert walls[0][0] == walls[1][0] == S.VALUE
    if gauges is not None:
        # the gauges change no population; their own totals show them.  The one exception is the header's: under open
        # ends nothing crosses the link right of column nx - 1
        assert np.array_equal(Run(nx, ny, ends, up, src, None, walls).g, base.g)
        for k, X in enumerate(gauges.stations):
            closed = ends is not None and X == nx - 1
            assert np.all((base.sums.right[k] == 0.0) == closed) and np.all((base.sums.left[k] == 0.0) == closed), X
        assert base.sums.up.size and np.all(base.sums.up != 0.0) and np.all(base.sums.down != 0.0)

    # every slot is visible
    if walls[0] != walls[1] or src is not None or up is not None:
        # (no flux / no flux without a source and without an uptake holds nothing per wall: there is no slot to tell)
        up2, src2, walls2 = mirrored_walls(up, src, walls)
        assert base.differs_from(Run(nx, ny, ends, up2, src2, gauges, walls2)), "the two walls swapped"
    if ends is not None and ends.kind[0] != ends.kind[1]:
        swapped = E.Ends(ends.kind[::-1], ends.value[::-1], ends.profile[::-1])
        assert base.differs_from(Run(nx, ny, swapped, up, src, gauges, walls)), "the two ends swapped"
    if ends is not None and ends.kind == (E.VALUE, E.VALUE):  # the same kind, two values
        swapped = E.Ends(ends.kind, ends.value[::-1], ends.profile[::-1])
        assert base.differs_from(Run(nx, ny, swapped, up, src, gauges, walls)), "the two ends' values swapped"
    if up is not None and all(r is not None for r in up.rate):
        assert base.differs_from(Run(nx, ny, ends, U.Uptake(up.rate[::-1]), src, gauges, walls)), "the two rates swapped"


def test_the_sets_are_what_they_claim():
    assert len(M.COMBOS) == len(set(M.COMBOS)) == 16 and all(len(c) == 4 for c in M.COMBOS)
    assert [M.WALLS[w] for w in M.WALL_NAMES] == [
        ((S.NOFLUX, 0.0), (S.NOFLUX, 0.0)), ((S.VALUE, 0.25), (S.NOFLUX, 0.0)), ((S.NOFLUX, 0.0), (S.VALUE, 0.4)),
        ((S.VALUE, 0.25), (S.VALUE, 1.75))]
    assert len(set(M.END_PAIRS)) == 9 and set(k for p in M.END_PAIRS for k in p) == set(E.KINDS)
    assert M.LATTICES_FULL == [(1, 2), (5, 257)] and M.LATTICES_ROTATED == [(2, 3), (33, 70)]
    assert len(M.matrix()) == len(set(M.matrix())) == 2 * 64 + 2 * 16
    assert sorted(M.orders()) == sorted(itertools.permutations(("source", "uptake", "ends", "gauges")))
    assert len(set(M.orders())) == 24


def test_coverage_is_complete():
    """Over the cases the GPU file runs."""
    cells, gauged, ungauged, under_value = {}, set(), set(), set()
    for nx, ny, ci, w in M.matrix():
        combo = M.COMBOS[ci]
        ends, up, src, gauges, walls = M.case(nx, ny, combo, w)
        cells.setdefault((nx, ny), set()).add((ci, w))
        if ends is not None:
            pair = tuple({v: k for k, v in E.KINDS.items()}[k] for k in ends.kind)
            (gauged if gauges is not None else ungauged).add(pair)
            if walls[1][0] == S.VALUE:
                under_value.update((side, pair[side]) for side in range(2))
    every_cell = {(ci, w) for ci in range(16) for w in M.WALL_NAMES}
    for size in M.LATTICES_FULL:  # every combination meets all four wall pairs, on each of these sizes
        assert cells[size] == every_cell and len(every_cell) == 64
    for size in M.LATTICES_ROTATED:
        assert {ci for ci, _ in cells[size]} == set(range(16)) and {w for _, w in cells[size]} == set(M.WALL_NAMES)
    assert gauged == set(M.END_PAIRS) and ungauged == set(M.END_PAIRS)
    assert under_value == {(side, kind) for side in range(2) for kind in E.KINDS}
    print(f"{len(M.matrix())} cases; all 64 combination x wall cells on {M.LATTICES_FULL}; end pairs with gauges "
          f"{sorted(gauged)}, without {sorted(ungauged)}")


@pytest.mark.parametrize("nx,ny", M.LATTICES_FULL + M.LATTICES_ROTATED)
def test_the_cases_keep_the_argument_rules(nx, ny):
    """What include/iblb.h refuses is never given, a per-column or per-row array stands wherever one may, and the two
    slots of every pair hold different numbers."""
    for ci, w in M.full_cells():
        ends, up, src, gauges, walls = M.case(nx, ny, M.COMBOS[ci], w)
        assert walls == M.WALLS[w]
        assert M.case(nx, ny, M.COMBOS[ci], w) is M.case(nx, ny, list(M.COMBOS[ci]), w)  # computed once
        noflux = [walls[k][0] == S.NOFLUX for k in range(2)]
        if src is not None:
            assert src.decay == 0.02 and src.source.shape == (ny, nx) and np.any(src.source != 0.0)
            for k in range(2):
                assert (src.wall_flux[k] is not None) == noflux[k] and (src.wall_value[k] is not None) == (not noflux[k])
                given = src.wall_flux[k] if noflux[k] else src.wall_value[k]
                assert given.shape == (nx,) and np.all(given != 0.0) and np.all(given != walls[k][1])
            assert src.present() == 3 | sum((4 if noflux[k] else 16) << k for k in range(2))
        if up is not None:
            for k in range(2):
                assert (up.rate[k] is not None) == noflux[k]
                assert up.rate[k] is None or (up.rate[k].shape == (nx,) and np.all((0.0 <= up.rate[k]) & (up.rate[k] < 2.0)))
        if ends is not None:
            assert ends.value == M.END_VALUES and ends.value[0] != ends.value[1]
            kinds = [k for k in range(2) if ends.kind[k] == E.VALUE]
            assert all(ends.profile[k] is None for k in range(2) if k not in kinds)
            assert sum(ends.profile[k] is not None for k in kinds) <= 1
            if len(kinds) == 2:  # a profile on one side, the uniform value on the other
                assert sum(ends.profile[k] is not None for k in kinds) == 1
            for k in kinds:
                assert ends.profile[k] is None or ends.profile[k].shape == (ny,)
        if gauges is not None:
            assert gauges.stations == tuple(sorted({0, nx // 2, nx - 1}))
            assert gauges.levels == tuple(sorted({0, (ny - 1) // 2, ny - 2}))
            assert all(0 <= x < nx for x in gauges.stations) and all(0 <= y <= ny - 2 for y in gauges.levels)
    if (nx, ny) == (1, 2):
        assert M.gauges_of(1, 2).stations == (0,) and M.gauges_of(1, 2).levels == (0,)


def test_both_kinds_of_value_end_are_met():
    """Over the matrix a value end takes a per-row profile and takes the uniform value, at each side."""
    met = set()
    for nx, ny, ci, w in M.matrix():
        ends = M.case(nx, ny, M.COMBOS[ci], w)[0]
        if ends is not None:
            met.update((k, ends.profile[k] is not None) for k in range(2) if ends.kind[k] == E.VALUE)
    assert met == {(0, False), (0, True), (1, False), (1, True)}
