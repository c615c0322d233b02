"""An independent restatement of the deep sweep's launch plan for tests/test_deep_plan.py, written from
DESIGN.md §4 (the deep sweep's prose and its build table), not from csrc/deep_plan.h.

A wave has 64 lanes of vs cells; each of the K levels invalidates one more row at each wave edge, so a
wave gives up ceil((K-1)/vs) lanes per edge.  The wall split walks the two wall-row chunks one cell per
lane: the bottom one owns one such wave's rows, the top one the last rows from an even row on."""

# MODE bits by name (iblb_timing.deep_mode reports their sum; nontemporal stores are in every build)
NT, SPLIT, PACK, SKIP, PRESHIFT, WINDOW = 1, 16, 64, 128, 256, 512


def owned_rows(K, vs):
    ghost = -(-(K - 1) // vs)
    return (64 - 2 * ghost) * vs


def split_rows(K, ny):
    """(rows of the bottom wall chunk, first row of the top wall chunk): the top chunk holds the last
    own1 rows, or one fewer so that it starts on an even row."""
    own1 = owned_rows(K, 1)
    top = ny - own1
    return own1, top + (top & 1)


def builds(f32, vs, slab):
    """DESIGN §4's table, row by row: the (MODE, waves per SIMD) pairs that exist."""
    if not f32 and vs == 2:
        row = [(785, 1), (273, 1), (129, 1), (1, 1)]
    elif not f32:
        row = [(1, 1), (129, 1)]
    elif vs == 2:
        row = ([] if slab else [(593, 3)]) + [(81, 2), (273, 3), (129, 1), (65, 1), (1, 1)]
    else:
        row = [(273, 4), (129, 1), (1, 1)] + ([] if slab else [(401, 3)])
    return set(row)


def choose(f32, vs, slab, K, ny, nskip, split, pack, window):
    """{mode, wpe, nch, wall_top, wall_ch0} by the table's columns: tall without skip regions, with skip
    regions, shorter than two wall chunks (or the split not asked for)."""
    rows = owned_rows(K, vs)
    own1, top = split_rows(K, ny)
    out = dict(nch=-(-ny // rows), wall_top=0, wall_ch0=0)
    tall = top > own1  # inner rows between the two wall chunks
    can_split = split and tall and (vs == 2 or f32)  # (the f64 one-cell split is not built)
    if can_split and nskip > 0 and not (f32 and vs == 1 and not slab):
        can_split = False  # only f32 with one cell per lane, no ghost columns, has a split build with skip regions
    if can_split:
        out.update(wall_top=top, wall_ch0=-(-(top - own1) // rows))
        if not f32:
            mode, wpe = NT + SPLIT + PRESHIFT + (WINDOW if window else 0), 1
        elif vs == 2:
            if pack and window and not slab:
                mode, wpe = NT + SPLIT + PACK + WINDOW, 3
            elif pack:
                mode, wpe = NT + SPLIT + PACK, 2
            else:
                mode, wpe = NT + SPLIT + PRESHIFT, 3
        elif nskip > 0:
            mode, wpe = NT + SPLIT + PRESHIFT + SKIP, 3
        else:
            mode, wpe = NT + SPLIT + PRESHIFT, 4
    elif nskip > 0:
        mode, wpe = NT + SKIP, 1
    elif f32 and vs == 2 and pack:
        mode, wpe = NT + PACK, 1
    else:
        mode, wpe = NT, 1
    out.update(mode=mode, wpe=wpe)
    return out


def edge_count(ranges, wait_lo, wait_hi):
    """Sweeps whose output columns reach below wait_lo or above wait_hi, by enumeration."""
    return sum(1 for xa, xb in ranges if any(x < wait_lo or x >= wait_hi for x in range(xa, xb)))


def call_pieces(K, r, depth_of):
    """The deep launches of a call of r iterations as step_range takes them: a launch of depth_of(left)
    while at least K - 1 iterations are left (and the launch fits).  Returns (pieces, left over)."""
    pieces = []
    while r >= K - 1:
        d = depth_of(r)
        if d > r:
            break
        pieces.append(d)
        r -= d
    return pieces, r
