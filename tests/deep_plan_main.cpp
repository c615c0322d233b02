// deep_plan_main.cpp — the deep sweep's launch planner (csrc/deep_plan.h) as a stand-alone CPU program
// for tests/test_deep_plan.py (TEST INFRASTRUCTURE; built by oracle/Makefile.san under ASan + UBSan).
// Reads whitespace-separated cases from stdin and prints one JSON line per case:
//   builds f32 vs slab
//   choose f32 vs slab K nskip split pack window ny_lo ny_hi     (one choice per ny in [ny_lo, ny_hi])
//   sweeps split vs col_begin col_end col_step W nsweep nch wall_ch0 slots wait_lo wait_hi
//   depth  K r_lo r_hi                                            (deep_depth(K, r) per r in [r_lo, r_hi])
//   parse  word
#include <cstdio>
#include <iostream>
#include <string>

#include "../cuda_iblb_11_amd/csrc/deep_plan.h"

using namespace iblb;

static bool builds_case() {
    int f32, vs, slab;
    if (!(std::cin >> f32 >> vs >> slab)) return false;
    const DeepBuilds l = deep_builds(f32 != 0, vs, slab != 0);
    std::printf("{\"builds\":[");
    for (int i = 0; i < l.n; ++i) std::printf("%s[%d,%d]", i ? "," : "", l.k[i].mode, l.k[i].wpe);
    std::printf("]}\n");
    return true;
}

static bool choose_case() {
    int f32, vs, slab, K, nskip, split, pack, window, ny_lo, ny_hi;
    if (!(std::cin >> f32 >> vs >> slab >> K >> nskip >> split >> pack >> window >> ny_lo >> ny_hi)) return false;
    if (K < 1 || vs < 1 || ny_lo < 1) return false;
    std::printf("{\"own1\":%d,\"rows_per_wave\":%d,\"ghost\":%d,\"c\":[", wall_own1(K), rows_per_wave(K, vs),
                ghost_lanes(K, vs));
    for (int ny = ny_lo; ny <= ny_hi; ++ny) {
        const DeepChoice c = deep_choose(f32 != 0, vs, slab != 0, K, ny, nskip, DeepBuild{split != 0, pack != 0, window != 0});
        std::printf("%s[%d,%d,%d,%d,%d]", ny > ny_lo ? "," : "", c.mode, c.wpe, c.nch, c.wall_top, c.wall_ch0);
    }
    std::printf("]}\n");
    return true;
}

static void ranges(const char* name, int cb, int ce, int step, int W, int nsw) {
    std::printf("\"%s\":[", name);
    for (int sw = 0; sw < nsw; ++sw) {
        const ColRange r = sweep_range(cb, ce, step, W, sw, nsw);
        std::printf("%s[%d,%d]", sw ? "," : "", r.xa, r.xb);
    }
    std::printf("]");
}

static bool sweeps_case() {
    int split, vs, cb, ce, step, W, nsweep, nch, ch0, wait_lo, wait_hi;
    long slots;
    if (!(std::cin >> split >> vs >> cb >> ce >> step >> W >> nsweep >> nch >> ch0 >> slots >> wait_lo >> wait_hi)) return false;
    if (W < 1 || ce <= cb || nch < 1 || (split && ch0 < 1)) return false;
    const DeepSweeps p = deep_sweeps(split != 0, vs, cb, ce, step, W, nsweep, nch, ch0, slots);
    const int e = deep_edge_waves(split != 0, cb, ce, step, W, p.nsweep, p.nsweep_w, nch, ch0, wait_lo, wait_hi);
    std::printf("{\"nsweep\":%d,\"nsweep_w\":%d,\"waves\":%ld,\"rounds\":%ld,\"edge_waves\":%d,", p.nsweep, p.nsweep_w,
                p.waves, p.rounds, e);
    ranges("ranges", cb, ce, step, W, p.nsweep);
    std::printf(",");
    ranges("ranges_w", cb, ce, step, W, p.nsweep_w);
    std::printf("}\n");
    return true;
}

static bool depth_case() {
    int K, r_lo, r_hi;
    if (!(std::cin >> K >> r_lo >> r_hi) || K < 1 || r_lo < 0) return false;
    std::printf("{\"d\":[");
    for (int r = r_lo; r <= r_hi; ++r) std::printf("%s%d", r > r_lo ? "," : "", deep_depth(K, r));
    std::printf("]}\n");
    return true;
}

static bool parse_case() {
    std::string w;
    if (!(std::cin >> w)) return false;
    DeepBuild b{true, true, true};  // (an unknown word leaves *out as it was)
    const bool ok = parse_deep_build(w.c_str(), &b);
    std::printf("{\"ok\":%d,\"split\":%d,\"pack\":%d,\"window\":%d}\n", (int)ok, (int)b.split, (int)b.pack, (int)b.window);
    return true;
}

int main() {
    std::string kind;
    while (std::cin >> kind) {
        const bool ok = kind == "builds"   ? builds_case()
                        : kind == "choose" ? choose_case()
                        : kind == "sweeps" ? sweeps_case()
                        : kind == "depth"  ? depth_case()
                        : kind == "parse"  ? parse_case()
                                           : false;
        if (!ok) {
            std::fprintf(stderr, "deep_plan_main: bad input\n");
            return 2;
        }
    }
    return 0;
}
