"""TEST INFRASTRUCTURE: the cases of the passive scalar's build matrix (pure numpy): every combination of a source, an
uptake, open ends and gauges, crossed with the four pairs of wall kinds, on lattices chosen for their edges.
tests/test_scalar_matrix.py pins the cases on the CPU (every switched-on feature and every slot shows in the
restatement's output, and the sets below cover what they claim); tests/test_gpu_scalar_matrix.py runs them on the GPU
against the twin.

The four features are the compile-time switches of scalar_push (csrc/scalar_kernels.hip): a combination is one build
of scalar_first_kernel<double>, scalar_first_kernel<float> and scalar_next_kernel, chosen at the launch by which device
arrays are set.
"""
import itertools

import numpy as np

import scalar_ref as S
import scalar_source_ref as Q
import scalar_uptake_ref as U
import scalar_ends_ref as E
import scalar_gauges_ref as G

# (source, uptake, ends, gauges); the index ci of a combination is 8 source + 4 uptake + 2 ends + gauges
COMBOS = list(itertools.product((False, True), repeat=4))

# four distinct values, so that a swapped slot shows
WALLS = {
    "no flux / no flux": S.NO_FLUX_WALLS,
    "value 0.25 / no flux": ((S.VALUE, 0.25), (S.NOFLUX, 0.0)),
    "no flux / value 0.4": ((S.NOFLUX, 0.0), (S.VALUE, 0.4)),
    "value 0.25 / value 1.75": ((S.VALUE, 0.25), (S.VALUE, 1.75)),
}
WALL_NAMES = list(WALLS)

END_PAIRS = list(itertools.product(("noflux", "value", "outflow"), repeat=2))  # (left, right)
END_VALUES = (0.8, 0.1)  # the uniform values, left and right: those of tests/test_gpu_scalar_ends.py

# 1 x 2: one column is its own left and right neighbour and one lane writes both ends' entries; the two wall rows are
# adjacent, there is one level, and the up-store and the down-store of a column land on each other's wall row.
# 5 x 257: the top wall row y = 256 sits alone in the second workgroup, and the level ny - 2 = 255 has its `up` writer
# and its `down` writer in different workgroups.
LATTICES_FULL = [(1, 2), (5, 257)]
# 2 x 3: both x-neighbours of a column are the same column.  33 x 70: one column more than the 32-wide transpose tile,
# six rows more than a 64-lane wave.
LATTICES_ROTATED = [(2, 3), (33, 70)]

SEED = 5
DECAY = 0.02


def combo_name(combo):
    return "".join(c for c, on in zip("SUEG", combo) if on) or "plain"


def case_id(nx, ny, ci, walls_name):
    """The test id of one case, e.g. 5x257-SEG-value_noflux."""
    kinds = "_".join("value" if k == S.VALUE else "noflux" for k, _ in WALLS[walls_name])
    return f"{nx}x{ny}-{combo_name(COMBOS[ci])}-{kinds}"


def end_pair(ci, wi):
    """The ends' kinds of combination ci under the wall pair wi: over the combinations with ends and the four wall
    pairs this reaches all nine pairs, with gauges and without (tests/test_scalar_matrix.py)."""
    return END_PAIRS[(ci + 3 * wi) % 9]


def full_cells():
    """Every combination under every wall pair: [(ci, walls_name)], 64 of them."""
    return [(ci, w) for ci in range(16) for w in WALL_NAMES]


def rotated_cells():
    """Every combination under one wall pair, WALLS[ci % 4]: [(ci, walls_name)], 16 of them."""
    return [(ci, WALL_NAMES[ci % 4]) for ci in range(16)]


def matrix():
    """The cases both test files run: [(nx, ny, ci, walls_name)], 2 x 64 + 2 x 16 = 160 of them."""
    return ([(nx, ny, ci, w) for nx, ny in LATTICES_FULL for ci, w in full_cells()] +
            [(nx, ny, ci, w) for nx, ny in LATTICES_ROTATED for ci, w in rotated_cells()])


def gauges_of(nx, ny):
    return G.Gauges(sorted({0, nx // 2, nx - 1}), sorted({0, (ny - 1) // 2, ny - 2}))


_CASES = {}


def case(nx, ny, combo, walls_name, seed=SEED):
    """(Ends, Uptake, Source, Gauges, walls) of one case, each None where the combination has it switched off;
    computed once, the arrays read-only.  The arguments keep the rules of include/iblb.h: a wall_flux and a rate only
    at a _NOFLUX wall, a wall_value only at a _VALUE wall, a profile only at a value end."""
    combo = tuple(bool(b) for b in combo)
    key = (nx, ny, combo, walls_name, seed)
    if key in _CASES:
        return _CASES[key]
    ci, wi = COMBOS.index(combo), WALL_NAMES.index(walls_name)
    walls = WALLS[walls_name]
    rng = np.random.default_rng([seed, nx, ny, ci, wi])
    arrays = []

    def keep(a):
        a.setflags(write=False)
        arrays.append(a)
        return a

    # drawn whether used or not, so that a case's arrays do not depend on which features are on
    field = keep(rng.uniform(-2e-3, 4e-3, (ny, nx)))
    flux = [keep(rng.uniform(-3e-3, 3e-3, nx)) for _ in range(2)]
    wall_value = [keep(walls[k][1] * rng.uniform(0.8, 1.2, nx)) for k in range(2)]
    rate = [keep(rng.uniform(0.0, 2.0, nx)) for _ in range(2)]
    profile = [keep(0.5 + 0.4 * np.sin(2.0 * np.pi * (np.arange(ny) + 0.5) / ny)), keep(rng.uniform(0.0, 1.0, ny))]
    noflux = [walls[k][0] == S.NOFLUX for k in range(2)]

    src = up = ends = gauges = None
    if combo[0]:
        src = Q.Source(field, DECAY, tuple(flux[k] if noflux[k] else None for k in range(2)),
                       tuple(None if noflux[k] else wall_value[k] for k in range(2)))
    if combo[1]:  # value / value: both rates None, the uptake only accumulates
        up = U.Uptake(tuple(rate[k] if noflux[k] else None for k in range(2)))
    if combo[2]:
        kinds = end_pair(ci, wi)
        side = (ci + wi) % 2  # the side whose value end takes a profile; the other side's takes the uniform value
        ends = E.Ends(kinds, END_VALUES, tuple(profile[k] if kinds[k] == "value" and k == side else None
                                               for k in range(2)))
    if combo[3]:
        gauges = gauges_of(nx, ny)
    _CASES[key] = (ends, up, src, gauges, walls)
    return _CASES[key]


def orders():
    """The 24 orders of the four iblb_set_scalar_* calls."""
    return list(itertools.permutations(("source", "uptake", "ends", "gauges")))
