// deep_plan.h — the host decisions of a deep-sweep launch (sweepk_kernel, lbm_sweep_impl.h): the row
// geometry, which kernel builds exist and which one a launch takes, how many sweeps and waves it gets,
// how many of its waves are edge waves, the depth mix of a call, and whether the collide's build for a
// body force along x only applies (tests/deep_force_main.cpp).  Pure functions, standard C++
// only: no HIP, no Sweep2Args, so that a CPU build can check them (tests/deep_plan_main.cpp,
// tests/test_deep_plan.py).  lbm_sweep_impl.h's launchers apply them and own the occupancy query and
// the launch; sweepk_kernel restates sweep_range and the row split on the device (the two must agree:
// the kernel's range arithmetic is kept as it is so that its code does not move).
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <string>

namespace iblb {

// The deep sweep's build features (deep_choose picks the kernel build from them; one that does not
// apply to a (type, cells per lane, layout) combination is ignored)
struct DeepBuild {
    bool split;   // the wall-row chunks as their own sweep family (one cell per lane), the inner chunks preshifted
    bool pack;    // f32, two cells per lane: both cells' collides as one packed f32x2 computation
    bool window;  // two cells per lane, split: the moving populations wait in an LDS window
    // not a feature of deep_choose's: the collide's force axis (below) held at the general build
    bool general_force = false;
};

// sweep only (MODE bits 1, 2, 4 as in lbm_vec.h; bit 0, nontemporal stores, is in every deep build):
// no software prefetch of the next column (two-step sweeps); the deep sweep's builds (sweepk_kernel).
// iblb_timing.deep_mode reports these numbers.
enum { MODE_NO_PREFETCH = 8, MODE_SPLIT = 16, MODE_PACK = 64, MODE_SKIP = 128, MODE_PRESHIFT = 256, MODE_LDSWIN = 512,
       MODE_WT_STORE = 1024 };

// ---- row geometry ----
// G ghost lanes at each wave edge (G * vs >= K - 1 rows: each level invalidates one more row)
constexpr int ghost_lanes(int K, int vs) { return (K - 1 + vs - 1) / vs; }
// owned rows of a wave with vs cells per lane
constexpr int rows_per_wave(int K, int vs) { return (64 - 2 * ghost_lanes(K, vs)) * vs; }
// row chunks (waves per sweep) of an unsplit launch
constexpr int deep_nch(int K, int vs, int ny) { return (ny + rows_per_wave(K, vs) - 1) / rows_per_wave(K, vs); }
// The wall split's rows: [0, OWN1) bottom wall chunk (one wave of one cell per lane), inner chunks of
// rows_per_wave from OWN1, top wall chunk from an even row (two-cell lanes of the inner chunks never
// straddle it) holding the last OWN1 or fewer rows
constexpr int wall_own1(int K) { return rows_per_wave(K, 1); }
constexpr int wall_top(int K, int ny) { return (ny - wall_own1(K) + 1) & ~1; }
constexpr int wall_ch0(int K, int vs, int top) {
    return (top - wall_own1(K) + rows_per_wave(K, vs) - 1) / rows_per_wave(K, vs);
}

// ---- the builds ----
struct DeepKernel {
    int mode, wpe;  // sweepk_kernel's MODE and waves-per-SIMD template arguments
};
struct DeepBuilds {
    int n;
    DeepKernel k[6];
};

// The sweepk_kernel builds of one (type, cells per lane, layout), at every depth: the only ones that
// exist (the launcher instantiates this list and nothing else; DESIGN.md §4 has it as a table).
constexpr DeepBuilds deep_builds(bool f32, int vs, bool slab) {
    constexpr int SPLIT = 1 | MODE_SPLIT | MODE_PRESHIFT;
    DeepBuilds l{0, {}};
    if (!f32 && vs == 2) {
        l.k[l.n++] = {SPLIT | MODE_LDSWIN, 1};
        l.k[l.n++] = {SPLIT, 1};
    }
    if (f32 && vs == 2) {
        if (!slab) l.k[l.n++] = {1 | MODE_SPLIT | MODE_PACK | MODE_LDSWIN, 3};
        l.k[l.n++] = {1 | MODE_SPLIT | MODE_PACK, 2};
        l.k[l.n++] = {SPLIT, 3};
        l.k[l.n++] = {1 | MODE_PACK, 1};
    }
    if (f32 && vs == 1) {
        if (!slab) l.k[l.n++] = {SPLIT | MODE_SKIP, 3};
        l.k[l.n++] = {SPLIT, 4};
    }
    l.k[l.n++] = {1 | MODE_SKIP, 1};
    l.k[l.n++] = {1, 1};
    return l;
}

struct DeepChoice {
    int mode, wpe;           // the build
    int nch;                 // row chunks of an unsplit launch
    int wall_top, wall_ch0;  // split builds: first row of the top wall chunk, inner chunks (else 0)
};

// The build of one (type, cells per lane, depth, layout) for the features asked; a feature that does
// not apply here is ignored.
inline DeepChoice deep_choose(bool f32, int vs, bool slab, int K, int ny, int nskip, DeepBuild build) {
    DeepChoice c{1, 1, deep_nch(K, vs, ny), 0, 0};
    // The wall split: two cells per lane in the inner chunks, and f32 with one (a group slab)
    if (vs == 2 || f32) {
        const int top = wall_top(K, ny);
        // f32, one cell per lane (a group slab's band cycle): the split with the skip regions too
        const bool split_skip = f32 && vs == 1 && !slab;
        if (build.split && (nskip == 0 || split_skip) && top > wall_own1(K)) {
            c.wall_top = top;
            c.wall_ch0 = wall_ch0(K, vs, top);
            c.mode = 1 | MODE_SPLIT | MODE_PRESHIFT;
            // waves per SIMD: f32 three at two cells per lane, four at one; f64 one
            c.wpe = f32 ? (vs == 2 ? 3 : 4) : 1;
            if (split_skip && nskip > 0) {  // three waves per SIMD (four: 6 dwords of scratch spills)
                c.mode |= MODE_SKIP;
                c.wpe = 3;
            } else if (f32 && vs == 2 && build.pack) {
                if (!slab && build.window) {
                    // the window (round 5): two of the three moving populations in LDS, three waves per SIMD
                    c.mode = 1 | MODE_SPLIT | MODE_PACK | MODE_LDSWIN;
                } else {
                    // the inner chunks packed, two waves per SIMD (the packed inner walk needs 191 VGPRs; forced
                    // to three waves it spills 21 dwords: 0.417 vs 0.323 ms per M f32 launch, profiles/r04/pack)
                    c.mode = 1 | MODE_SPLIT | MODE_PACK;
                    c.wpe = 2;
                }
            } else if (!f32 && build.window) {  // (vs == 2) the LDS window of the inner chunks
                c.mode |= MODE_LDSWIN;
            }
            return c;
        }
    }
    // the IB band cycle's deep and boundary sweeps beside its last level: patch output rows left out
    if (nskip > 0) c.mode = 1 | MODE_SKIP;
    else if (f32 && vs == 2 && build.pack) c.mode = 1 | MODE_PACK;
    // (else the plain walk: the preshift in every chunk, without the split, is slower: M f64 0.559 vs 0.521 ms
    // per launch, profiles/r04/split64: the wall waves, which set the launch time, wait on the wall rows'
    // uniform loads; with the split the inner chunks take it and the wall waves have slack)
    return c;
}

// ---- sweeps ----
// wall split: sweeps of a wall chunk per sweep of an inner chunk, in quarters.  With one-cell wall
// walks (no spills) the launch time is the inner waves' whatever the ratio: M f32 0.319-0.322 ms per
// launch for 0.5 ... 1.5 (profiles/r03s1); the first split (two-cell wall walks with spills) needed 2
// (0.305-0.320 ms, profiles/r03sp, r03r2).
constexpr int WALL_SWEEPS_X4 = 4;

struct DeepSweeps {
    int nsweep, nsweep_w;  // sweeps of each chunk (split: of each inner chunk), of each wall chunk (split only)
    long waves;
    long rounds;           // balanced sweeps with `slots` known: the device-wide rounds aimed at (else 0)
};

// The sweeps and waves of a launch over columns [col_begin, col_end).  col_step > 0: `nsweep` fixed
// sweeps as given (a slab's boundary sweeps), the wall chunks too.  col_step <= 0, balanced sweeps: the
// wave count a whole number of device-wide rounds of `slots` resident waves (the waves of one launch all
// do the same work, so a partial last round idles the chip; slots 0: unknown, no rounding), sweeps close
// to the requested W columns.  split: wall_ch0 inner chunks, and the two wall chunks with r sweeps
// per inner sweep.
inline DeepSweeps deep_sweeps(bool split, int vs, int col_begin, int col_end, int col_step, int W, int nsweep, int nch,
                              int wall_ch0, long slots) {
    DeepSweeps p{nsweep, 0, 0, 0};
    if (col_step <= 0) {
        const long n = col_end - col_begin;
        long ns = (n + W - 1) / W;
        if (split) {
            const long nin = wall_ch0, r4 = vs == 1 ? 6 : WALL_SWEEPS_X4;  // vs 1: wall walks ~1.4x the inner
            if (slots > 0) {
                p.rounds = std::max(1L, (ns * (4 * nin + 2 * r4) / 4 + slots / 2) / slots);
                ns = std::max(1L, 4 * p.rounds * slots / (4 * nin + 2 * r4));
            }
            p.nsweep = (int)std::min(ns, n);
            p.nsweep_w = (int)std::min((ns * r4 + 3) / 4, n);
        } else {
            if (slots > 0) {
                p.rounds = std::max(1L, (ns * nch + slots / 2) / slots);
                ns = std::max(1L, p.rounds * slots / nch);
            }
            p.nsweep = (int)std::min(ns, n);
        }
    } else if (split) {
        p.nsweep_w = nsweep;
    }
    p.waves = split ? (long)p.nsweep * wall_ch0 + 2L * p.nsweep_w : (long)p.nsweep * nch;
    return p;
}

struct ColRange {
    int xa, xb;  // output columns [xa, xb)
};

// The output columns of sweep sw of nsw (sweepk_kernel computes the same on the device).  col_step > 0:
// W columns from col_begin + sw * col_step, clipped at col_end; else balanced: nsw sweeps of
// floor/ceil((col_end - col_begin) / nsw) columns.
inline ColRange sweep_range(int col_begin, int col_end, int col_step, int W, int sw, int nsw) {
    if (col_step > 0) {
        const int xa = col_begin + sw * col_step;
        return {xa, std::min(xa + W, col_end)};
    }
    const long n = (long)(col_end - col_begin);
    return {col_begin + (int)(sw * n / nsw), col_begin + (int)((sw + 1) * n / nsw)};
}

// The waves of a launch that are edge waves (sweepk_kernel's `edge`: output columns reaching below
// wait_lo or above wait_hi; wait_lo = INT_MAX: every wave).  A slab's interior waits for as many
// counts of its done word, so this and the kernel must agree exactly.
inline int deep_edge_waves(bool split, int col_begin, int col_end, int col_step, int W, int nsweep, int nsweep_w, int nch,
                           int wall_ch0, int wait_lo, int wait_hi) {
    auto edges = [&](int nsw) {
        int e = 0;
        for (int sw = 0; sw < nsw; ++sw) {
            const ColRange r = sweep_range(col_begin, col_end, col_step, W, sw, nsw);
            e += (r.xa < wait_lo || r.xb > wait_hi) ? 1 : 0;
        }
        return e;
    };
    return split ? edges(nsweep) * wall_ch0 + 2 * edges(nsweep_w) : edges(nsweep) * nch;
}

// ---- a call's depths ----
// Depth of the next deep launch without IB, r >= K-1 iterations left in the call: K, or K-1 where
// launches of K-1 (j of them) leave a multiple of K, so that r = j (K-1) + m K needs no two-iteration
// or one-step remainder (every r >= (K-1)(K-2) qualifies: 20 = 4 x 5 at K = 6, 500 = 4 x 5 + 80 x 6).
// A remainder costs more than the depth: M f64 20 iterations at K = 6 as 3 x 6 + 2 took 0.111 ms per
// iteration against 0.097 as 4 x 5 (profiles/r04/depth).
inline int deep_depth(int K, int r) {
    if (K < 4) return K;
    const int j = (K - r % K) % K;
    return (j > 0 && (long)j * (K - 1) <= r) ? K - 1 : K;
}

// IBLB_DEEP_BUILD: a comma list of split, pack, window, or the one word plain (no feature)
inline bool parse_deep_build(const char* e, DeepBuild* out) {
    const std::string v(e);
    DeepBuild b{false, false, false};
    if (v != "plain")
        for (size_t i = 0; i <= v.size();) {
            const size_t j = std::min(v.find(',', i), v.size());
            const std::string w = v.substr(i, j - i);
            if (w == "split") b.split = true;
            else if (w == "pack") b.pack = true;
            else if (w == "window") b.window = true;
            else return false;
            i = j + 1;
        }
    *out = b;
    return true;
}

// ---- the collide's force axis ----
// The deep sweep's collide has a second build for a body force along x only (XF, relax_cells /
// relax_dev in iblb_device.h): the launcher takes it when the launch's force constants allow it.
// F_y = +0 or -0 does; a NaN or a denormal F_y does not.
constexpr bool deep_force_x_only(double fx, double fy) { return (void)fx, fy == 0.0; }

// IBLB_DEEP_FORCE: the one word general (the general collide whatever the force: the tests' and the
// same-library comparison's knob)
inline bool parse_deep_force(const char* e, bool* general) {
    if (std::string(e) != "general") return false;
    *general = true;
    return true;
}

}  // namespace iblb
