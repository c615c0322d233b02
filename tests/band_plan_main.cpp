// band_plan_main.cpp — the band planner (csrc/band_plan.h) as a stand-alone CPU program for
// tests/test_band_plan.py (TEST INFRASTRUCTURE; built by oracle/Makefile.san under ASan + UBSan).
// Reads whitespace-separated cases from stdin and prints one JSON line per case:
//   plan K nx ny x_begin ncol gc slab V f64 flux merged vhalf  nslab edge*nslab  npts (x y)*npts
//   arr  slab f64 K share deep_cols ny merge per_xcd
#include <cstdio>
#include <iostream>
#include <string>

#include "../cuda_iblb_11_amd/csrc/band_plan.h"

using namespace iblbh;

template <typename V>
static void ints(const char* name, const V& v, const char* end = ",") {
    std::printf("\"%s\":[", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? "," : "", (int)v[i]);
    std::printf("]%s", end);
}

template <typename V>
static void rows(const char* name, const V& v) {
    std::printf("\"%s\":[", name);
    for (size_t i = 0; i < v.size(); ++i) {
        std::printf("%s[", i ? "," : "");
        for (size_t k = 0; k < v[i].size(); ++k) std::printf("%s%d", k ? "," : "", v[i][k]);
        std::printf("]");
    }
    std::printf("],");
}

static bool plan_case() {
    BandGeom g;
    int slab, f64, merged, vhalf, nslab, npts;
    if (!(std::cin >> g.K >> g.nx >> g.ny >> g.x_begin >> g.ncol >> g.gc >> slab >> g.V >> f64 >> g.flux >> merged >>
          vhalf >> nslab))
        return false;
    g.slab = slab != 0;
    g.f64 = f64 != 0;
    std::vector<int> edges((size_t)nslab);
    for (int& e : edges) std::cin >> e;
    g.slab_begin = &edges;
    if (!(std::cin >> npts) || npts < 0) return false;
    std::vector<float> xy((size_t)2 * npts);
    for (float& v : xy) std::cin >> v;
    if (!std::cin || g.K < 1 || g.ncol < 1 || g.ny < 1 || g.gc < 0 || g.V < 2) return false;

    BandPatches pat = band_patches(g, xy);
    std::printf("{\"feasible\":%d,\"d\":%d,\"x\":%d,", (int)pat.feasible, pat.d, pat.x);
    if (!pat.feasible) {
        rows("b", pat.b);
        std::printf("\"end\":1}\n");
        return true;
    }
    const BandPlan p = band_tables(g, std::move(pat), merged != 0, vhalf != 0);
    rows("b", p.b);
    rows("pr", p.pr);
    ints("tab", p.tab);
    ints("off", p.off);
    ints("n", p.n);
    ints("nchl", p.nchl);
    std::printf("\"cells\":%lld,\"flux\":%d,\"fy0\":%d,\"fy1\":%d,\"too_big\":%d,\"merged\":%d,\"vhalf\":%d,", p.cells,
                p.flux, p.fy0, p.fy1, (int)p.too_big, (int)p.merged, (int)p.vhalf);
    std::vector<std::array<int, 4>> skip;
    for (const iblb::SkipBox& s : band_skip_boxes(g, p)) skip.push_back({s.x0, s.x1, s.y0, s.y1});
    rows("skip", skip);
    for (int mg = 0; mg < 2; ++mg) {  // force_clip of every level at the plan's ghost depth
        std::vector<std::array<int, 2>> clip((size_t)g.K);
        for (int j = 0; j < g.K; ++j) force_clip(g.K, p.d, g.ncol, j, mg != 0, &clip[j][0], &clip[j][1]);
        rows(mg ? "clip_merged" : "clip_chained", clip);
    }
    int wlo, whi;
    wrap_range(g.K, p.d, g.nx, g.x_begin, g.ncol, xy.data(), npts, &wlo, &whi);
    std::printf("\"wrap\":[%d,%d]}\n", wlo, whi);
    return true;
}

static bool arr_case() {
    int slab, f64, K, ny, merge, per_xcd;
    long long deep_cols;
    double share;
    if (!(std::cin >> slab >> f64 >> K >> share >> deep_cols >> ny >> merge >> per_xcd)) return false;
    const bool bound = chain_bound(K, deep_cols, ny, f64 != 0);
    const BandArrangement a = band_arrangement(slab != 0, f64 != 0, K, share, bound, merge, per_xcd);
    std::printf("{\"bound\":%d,\"merged\":%d,\"want\":%ld,\"own_build\":%d}\n", (int)bound,
                (int)chain_merged(merge, bound), a.want, (int)a.own_build);
    return true;
}

int main() {
    std::string kind;
    while (std::cin >> kind) {
        const bool ok = kind == "plan" ? plan_case() : kind == "arr" ? arr_case() : false;
        if (!ok) {
            std::fprintf(stderr, "band_plan_main: bad input\n");
            return 2;
        }
    }
    return 0;
}
