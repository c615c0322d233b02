// deep_force_main.cpp — the force axis of the deep sweep's collide (csrc/deep_plan.h: deep_force_x_only,
// IBLB_DEEP_FORCE) and the constants its x-only build leans on (csrc/iblb_device.h: make_kforce) as a
// stand-alone CPU program for tests/test_deep_force.py (TEST INFRASTRUCTURE; the test builds it host-only
// under ASan + UBSan and runs it as a child process; it makes no HIP call).
// Reads whitespace-separated cases from stdin and prints one JSON line per case; every floating-point
// value goes in and out as the hexadecimal bit pattern of a double (f32 results: of a float):
//   xonly  fx fy                      deep_force_x_only
//   word   text                       parse_deep_force
//   kforce f32 tau tau2 fx fy         make_kbase + make_kforce in double (f32 = 0) or float (1)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

#include "../cuda_iblb_11_amd/csrc/deep_plan.h"
#include "../cuda_iblb_11_amd/csrc/iblb_device.h"

using namespace iblb;

static bool read_double(double* v) {
    std::string w;
    if (!(std::cin >> w)) return false;
    const unsigned long long b = std::stoull(w, nullptr, 16);
    std::memcpy(v, &b, sizeof b);
    return true;
}
static unsigned long long bits(double v) {
    unsigned long long b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}
static unsigned long long bits(float v) {
    uint32_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

static bool xonly_case() {
    double fx, fy;
    if (!read_double(&fx) || !read_double(&fy)) return false;
    std::printf("{\"x_only\":%d}\n", deep_force_x_only(fx, fy) ? 1 : 0);
    return true;
}

static bool word_case() {
    std::string w;
    if (!(std::cin >> w)) return false;
    bool general = false;
    const bool ok = parse_deep_force(w == "-" ? "" : w.c_str(), &general);
    std::printf("{\"ok\":%d,\"general\":%d}\n", ok ? 1 : 0, general ? 1 : 0);
    return true;
}

template <typename R>
static void kforce_print(const Coef& c) {
    const KBase<R> b = make_kbase<R>(c);
    const KForce<R> k = make_kforce<R>(b, (R)c.gx, (R)c.gy);
    std::printf("{\"Fx\":\"%llx\",\"Fy\":\"%llx\",\"hFx\":\"%llx\",\"hFy\":\"%llx\",\"kwi4\":\"%llx\",\"kwi2\":\"%llx\"", bits(k.Fx),
                bits(k.Fy), bits(k.hFx), bits(k.hFy), bits(b.kwi4[1]), bits(b.kwi2[1]));
    for (int p = 0; p < 4; ++p) std::printf(",\"hE%d\":\"%llx\",\"gO%d\":\"%llx\"", p, bits(k.hE[p]), p, bits(k.gO[p]));
    std::printf("}\n");
}

static bool kforce_case() {
    int f32;
    double tau, tau2, fx, fy;
    if (!(std::cin >> f32) || !read_double(&tau) || !read_double(&tau2) || !read_double(&fx) || !read_double(&fy)) return false;
    if (!(tau > 0.5) || !(tau2 > 0.5)) return false;
    // (the context's Coef, iblb_ctx.hip:iblb_create)
    const double cs = 0.57735;
    Coef c;
    c.omega_p = 1. / tau;
    c.omega_m = 1. / tau2;
    c.kguo = 1. - 1. / (2. * tau);
    c.inv_cs2 = 1. / (cs * cs);
    c.inv_cs4 = 1. / (cs * cs * cs * cs);
    c.inv_2cs2 = 1. / (2 * cs * cs);
    c.inv_2cs4 = 1. / (2 * cs * cs * cs * cs);
    c.gx = fx;
    c.gy = fy;
    if (f32) kforce_print<float>(c);
    else kforce_print<double>(c);
    return true;
}

int main() {
    std::string op;
    while (std::cin >> op) {
        bool ok = false;
        if (op == "xonly") ok = xonly_case();
        else if (op == "word") ok = word_case();
        else if (op == "kforce") ok = kforce_case();
        if (!ok) {
            std::fprintf(stderr, "bad case: %s\n", op.c_str());
            return 2;
        }
    }
    return 0;
}
