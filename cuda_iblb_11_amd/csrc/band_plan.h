// band_plan.h — the IB band cycle's planner (ctx_band.hip's header comment has the cycle): pure
// functions of the slab's geometry and the points.  Host only, standard C++ only: no HIP, no context,
// no resources, so that a CPU build can check it (tests/band_plan_main.cpp, tests/test_band_plan.py).
// ctx_band.hip:plan_bands runs the stages in order and owns the streams, pinned slots and buffers.
#pragma once

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <utility>
#include <vector>

#include "skip_box.h"

namespace iblbh {

struct BandGeom {
    int K = 0;                    // the deep sweep's depth: iterations per cycle
    int nx = 0, ny = 0;           // the lattice
    int x_begin = 0, ncol = 0;    // the slab's own columns [x_begin, x_begin + ncol)
    int gc = 0;                   // ghost columns per side
    bool slab = false;            // a slab of a group (not a lone slab)
    const std::vector<int>* slab_begin = nullptr;  // the group's slab edges (global columns; slab only)
    int V = 2;                    // cells per lane of the level launches: 64 * V rows per chunk
    bool f64 = true;
    int flux = -1;                // the flux column (local) where the slab owns it, else -1
};

// stage 1: where the force acts
struct BandPatches {
    std::vector<std::array<int, 4>> b;  // patches {x0, x1, y0, y1}: forced columns and rows (local, inclusive)
    int d = 0;                          // ghost depth the trapezoids read (0: all inside the slab)
    int x = 0;                          // halo depth of the cycle's exchange (slab groups; same on every rank)
    bool feasible = true;
};

// stage 2 (and the glue's decisions): what the cycle's launches need
struct BandPlan {
    std::vector<std::array<int, 4>> b;  // as BandPatches
    int d = 0, x = 0;
    bool merged = false;                // the chain's flavour: each level's launch also evaluates the next level's force
    bool vhalf = false;                 // the level entries are in chunks of 64 * V/2 rows
    std::vector<std::array<int, 2>> pr; // a patch's output rows [pr0, pr1): even bounds (or ny)
    std::vector<int> tab;               // level tables: {column, first chunk, end chunk, pr0, pr1} per entry
    std::vector<int> off, n, nchl;      // level j: first entry, entries, chunks of its tallest entry
    long long cells = 0;                // cells of all trapezoid levels
    int flux = -1, fy0 = 0, fy1 = 0;    // flux column in a patch output, the patch's rows
    bool too_big = false;               // a lone slab's trapezoids over half the lattice: the cycle does not pay
    bool par = false;                   // the last level runs beside the deep sweep, which skips ...
    std::vector<iblb::SkipBox> skip;    // ... the patch output regions (own columns, rows pr)
};

// periodic distance from global column f to the nearest slab edge of the group
inline int edge_distance(const BandGeom& g, int f) {
    int best = INT_MAX;
    for (int e : *g.slab_begin) {
        int d = std::abs(f - e) % g.nx;
        best = std::min(best, std::min(d, g.nx - d));
    }
    return best;
}

// Stage 1: the patches from the (x, y) of every point the cycle may see.
inline BandPatches band_patches(const BandGeom& g, const std::vector<float>& xy) {
    const int K = g.K, R = 2 * (K - 1);
    const int ncol = g.ncol, ny = g.ny, nx = g.nx, D = g.gc;
    const int lo = -D + 1, hi = ncol + D - 2;  // level-0 columns a trapezoid may cover (local)
    const int W = ncol + 2 * D;
    // forced cells of every point image in [lo, hi]: a row range per local column (index x + D);
    // and whether any point forces a column near any slab edge (the group's exchange depth: every
    // rank holds every point, so every rank finds the same answer)
    std::vector<int> fy0((size_t)W, INT_MAX), fy1((size_t)W, INT_MIN);
    const int zone = std::max(D, R + 2);
    bool edge_any = false;
    // consecutive points in one column (a filament's) accumulate their rows in registers and update
    // the column table once: per-point updates of the same few entries chain through store-to-load
    // forwarding (768 points x K+1 iterations: 131 -> 24 us per plan on a container core)
    int cx = INT_MIN, cy0 = 0, cy1 = 0;
    auto flush = [&]() {
        if (cx == INT_MIN) return;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xg = cx + dx;  // forced global column (the spread has no periodic image)
            if (xg < 0 || xg >= nx) continue;
            if (g.slab && !edge_any && edge_distance(g, xg) <= zone) edge_any = true;
            for (int m = -1; m <= 1; ++m) {
                const int x = xg - g.x_begin + m * nx;
                if (x < lo || x > hi) continue;
                fy0[(size_t)(x + D)] = std::min(fy0[(size_t)(x + D)], cy0);
                fy1[(size_t)(x + D)] = std::max(fy1[(size_t)(x + D)], cy1);
            }
        }
    };
    for (size_t k = 0; k + 1 < xy.size(); k += 2) {
        const int x0 = (int)std::nearbyint((double)xy[k]);
        const int y0 = (int)std::nearbyint((double)xy[k + 1]);
        const int ya = std::min(std::max(0, y0 - 1), ny - 1), yb = std::max(std::min(ny - 1, y0 + 1), 0);
        if (x0 == cx) {
            cy0 = std::min(cy0, std::min(ya, yb));
            cy1 = std::max(cy1, std::max(ya, yb));
            continue;
        }
        flush();
        cx = x0;
        cy0 = std::min(ya, yb);
        cy1 = std::max(ya, yb);
    }
    flush();
    // forced column intervals with their row range, merged into patches {x0, x1, y0, y1} whose
    // trapezoids stay apart (gaps >= 2R + 8 columns)
    BandPatches p;
    std::vector<std::array<int, 4>>& b = p.b;
    for (int x = lo; x <= hi;) {
        if (fy0[(size_t)(x + D)] > fy1[(size_t)(x + D)]) { ++x; continue; }
        std::array<int, 4> iv{x, x, fy0[(size_t)(x + D)], fy1[(size_t)(x + D)]};
        while (iv[1] + 1 <= hi && fy0[(size_t)(iv[1] + 1 + D)] <= fy1[(size_t)(iv[1] + 1 + D)]) {
            ++iv[1];
            iv[2] = std::min(iv[2], fy0[(size_t)(iv[1] + D)]);
            iv[3] = std::max(iv[3], fy1[(size_t)(iv[1] + D)]);
        }
        if (!b.empty() && iv[0] - b.back()[1] - 1 < 2 * R + 8) {
            b.back()[1] = iv[1];
            b.back()[2] = std::min(b.back()[2], iv[2]);
            b.back()[3] = std::max(b.back()[3], iv[3]);
        } else {
            b.push_back(iv);
        }
        x = iv[1] + 1;
    }
    // ghosts: a trapezoid whose level-0 input [x0 - R - 1, x1 + R + 1] leaves the slab reads D
    // ghost columns (and the garbage frontier argument of ctx_band.hip needs all of them)
    bool need = false;
    for (auto& q : b) need |= q[0] - R - 1 < 0 || q[1] + R + 1 > ncol - 1;
    p.d = need ? D : 0;
    p.x = g.slab ? std::max(K, edge_any ? D : 0) : 0;
    p.feasible = !(need && (g.slab ? !edge_any : ncol < D));  // (cannot fail for a slab: need implies edge_any)
    return p;
}

// Stage 2: the level tables of the patches' trapezoids.
// Rows: a patch's output rows [ya, yb) = its forced rows +- (K-1); level j covers K-1-j more on
// each side (the deep sweep advances every row, the last level overwrites the output rows)
// (even bounds: a lane of the deep sweep's two-cell walk is then wholly in or out of a patch
// output, which the deep sweep leaves to the last level when the two run side by side)
inline BandPlan band_tables(const BandGeom& g, BandPatches&& pat, bool merged, bool vhalf) {
    const int K = g.K, R = 2 * (K - 1), ncol = g.ncol, ny = g.ny;
    BandPlan p;
    p.b = std::move(pat.b);
    p.d = pat.d;
    p.x = pat.x;
    p.merged = merged;
    p.vhalf = vhalf;
    const std::vector<std::array<int, 4>>& b = p.b;
    const int V64 = 64 * (vhalf ? g.V / 2 : g.V);  // rows per chunk of the level launches
    const int nchv = (ny + V64 - 1) / V64;         // such chunks per column
    p.pr.resize(b.size());
    for (size_t q = 0; q < b.size(); ++q)
        p.pr[q] = {std::max(0, b[q][2] - (K - 1)) & ~1, std::min(ny, (b[q][3] + K + 1) & ~1)};
    p.off.resize((size_t)K);
    p.n.resize((size_t)K);
    p.nchl.assign((size_t)K, 0);
    for (int j = 0; j < K; ++j) {
        p.off[j] = (int)p.tab.size();
        p.n[j] = 0;
        const int m = K - 1 - j;
        const int lj = -p.d + 1 + j, hj = ncol + p.d - 2 - j;  // columns level j can compute
        for (size_t q = 0; q < b.size(); ++q) {
            const int ylo = std::max(0, p.pr[q][0] - m), yhi = std::min(ny, p.pr[q][1] + m);
            const int ch0 = ylo / V64, ch1 = std::min(nchv, (yhi + V64 - 1) / V64);
            int xa = std::max(b[q][0] - R + j, lj), xb = std::min(b[q][1] + R - j, hj);
            if (j == K - 1) {  // the last level stores the slab's own columns only
                xa = std::max(xa, 0);
                xb = std::min(xb, ncol - 1);
            }
            if (xa > xb) continue;
            p.nchl[j] = std::max(p.nchl[j], ch1 - ch0);
            for (int x = xa; x <= xb; ++x) {
                p.tab.insert(p.tab.end(), {x, ch0, ch1, p.pr[q][0], p.pr[q][1]});
                ++p.n[j];
                p.cells += std::min(ny, ch1 * V64) - ch0 * V64;
            }
        }
    }
    p.too_big = !g.slab && 2 * p.cells > (long long)K * g.nx * ny;
    if (g.flux >= 0)
        for (size_t q = 0; q < b.size(); ++q)
            if (g.flux >= b[q][0] - (K - 1) && g.flux <= b[q][1] + (K - 1)) {
                p.flux = g.flux;
                p.fy0 = p.pr[q][0];
                p.fy1 = p.pr[q][1];
            }
    return p;
}

// Stage 3: the patch outputs — the last level's entries: own columns [x0 - (K-1), x1 + (K-1)],
// rows pr — for the deep sweep to skip.  Empty where those regions do not stay disjoint in columns
// (periodic images of a tiny slab could overlap) or do not fit the kernel arguments.
inline std::vector<iblb::SkipBox> band_skip_boxes(const BandGeom& g, const BandPlan& p) {
    std::vector<iblb::SkipBox> skip;
    if (p.b.size() > (size_t)iblb::MAX_SKIP) return skip;
    for (size_t q = 0; q < p.b.size(); ++q) {
        const int x0 = std::max(0, p.b[q][0] - (g.K - 1)), x1 = std::min(g.ncol - 1, p.b[q][1] + (g.K - 1));
        if (x0 > x1) continue;
        if (!skip.empty() && x0 <= skip.back().x1) return {};
        skip.push_back(iblb::SkipBox{x0, x1, p.pr[q][0], p.pr[q][1]});
    }
    return skip;
}

// Columns the force of level j may be spread into (the band trapezoid's [clo, chi)); D: the plan's
// ghost depth.  Chained levels: the columns level j computes; the last level stores the slab's own
// columns only, so a force left in a ghost column would never be consumed.  Merged chain: one
// column less at each ghost edge (the launch after a level clears that level's force at its own
// entries, one column narrower: the dropped column lies inside the garbage frontier, at level j
// columns up to -D+2+3j are garbage, §5 of DESIGN.md), and level K-2 only where the last level's
// cells and the nodes of its force pull: columns -3 .. ncol+2 (a point that forces column 0 has
// x0 >= -1, so its nodes start at x0-1 >= -2; their pulls reach -3, where the level's collide is
// recomputed, so the level's force is needed from column -3); the last launch clears those outside
// its own.
inline void force_clip(int K, int D, int ncol, int j, bool merged, int* clo, int* chi) {
    const int n = ncol;
    if (j == K - 1) {
        *clo = std::max(0, -D + 1 + j);
        *chi = std::min(n, n + D - 1 - j);
    } else if (!merged) {
        *clo = -D + 1 + j;
        *chi = n + D - 1 - j;
    } else if (j == K - 2) {
        *clo = std::max(-3, -D + 2 + j);
        *chi = std::min(n + 3, n + D - 2 - j);
    } else {
        *clo = -D + 2 + j;
        *chi = n + D - 2 - j;
    }
}

// Point indices [*lo, *hi) of the ns points xy that may have a periodic image (m = -1 / +1)
// spreading into the slab's trapezoid columns this cycle: a slab that touches the lattice's x edge,
// ghost trapezoids (D > 0), points within the trapezoids' reach of that edge at iteration t (the
// cycle moves them less than a column per iteration; the hint only balances the merged launches'
// point groups, every image is evaluated either way, band_level_kernel)
inline void wrap_range(int K, int D, int nx, int x_begin, int ncol, const float* xy, int ns, int* lo, int* hi) {
    *lo = *hi = 0;
    if (D <= 0 || ns <= 0 || !xy || (x_begin != 0 && x_begin + ncol != nx)) return;
    const int margin = D + 2 * K + 4;
    int a = INT_MAX, b = -1;
    for (int k = 0; k < ns; ++k) {
        const int x0 = (int)std::nearbyint((double)xy[2 * k]);
        if (x0 < margin || x0 > nx - 1 - margin) {
            a = std::min(a, k);
            b = k;
        }
    }
    if (b >= 0 && b + 1 - a < ns) {  // (every point: nothing to balance)
        *lo = a;
        *hi = b + 1;
    }
}

// The chain, not the deep sweep beside it, is the cycle's critical path: the deep sweep (deep_cols
// columns, K iterations, 130e3 / 190e3 cells per us in f64 / f32) is shorter than 1.5x a chain of
// 2K ~8 us launches (narrow slabs).  The criterion of the merged chain, of PAR and of the streams'
// arrangement.
inline bool chain_bound(int K, long long deep_cols, int ny, bool f64) {
    const double deep_us = (double)K * deep_cols * ny / (f64 ? 130e3 : 190e3);
    return deep_us < 1.5 * 2 * K * 8.0;
}

// the merged chain under the IBLB_BAND_MERGE setting (1 auto, 2 always, 0 never)
inline bool chain_merged(int merge, bool bound) { return merge == 2 || (merge == 1 && bound); }

// The streams' arrangement of the overlapped cycle (ctx_band.hip:band_streams, which has the
// measurements): CUs of the chain's stream (-2: both streams unmasked, the chain's at the highest
// priority) and whether the deep sweep runs in its own build beside it.  share: the trapezoids' part
// of the cycle's lattice updates; per_xcd: CUs of one XCD.
struct BandArrangement {
    long want;
    bool own_build;
};
inline BandArrangement band_arrangement(bool slab, bool f64, int K, double share, bool bound, int merge, int per_xcd) {
    BandArrangement a{(share > 0.05 ? 2 : 1) * (long)per_xcd, false};
    if (slab && chain_merged(merge, bound) && K >= 7) a.want = 2 * per_xcd;
    if (!slab && !bound) {
        if (!f64 && K >= 7) {
            a.want = per_xcd;
            a.own_build = true;
        } else {
            a.want = -2;
        }
    }
    return a;
}

}  // namespace iblbh
