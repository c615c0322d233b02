// ckpt_format_main.cpp — drives csrc/ckpt_format.h (the checkpoint's framing: pure host code) for
// tests/test_ckpt_format.py.  One command per line on stdin, one JSON object per line on stdout:
//   scan <fluid_end> <path>   iblbck::scan from fluid_end: status, and with status 0 the sections found
//   info <path>               iblbck::read_fluid_header, then the scan from the end it gives
// Built host-only, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../cuda_iblb_11_amd/csrc/ckpt_format.h"

using namespace iblbck;

static void print_scan(int status, const Scan& sc) {
    std::printf("\"status\": %d, \"message\": \"%s\", \"size\": %lld, \"observers\": %u, \"present\": [", status,
                scan_message(status), sc.file_bytes, status == SCAN_OK ? sc.observers() : 0u);
    for (int k = 0; k < N_KINDS; ++k) std::printf("%s%d", k ? ", " : "", status == SCAN_OK && sc.present[k] ? 1 : 0);
    std::printf("], \"offset\": [");
    for (int k = 0; k < N_KINDS; ++k) std::printf("%s%lld", k ? ", " : "", status == SCAN_OK ? sc.offset[k] : 0LL);
    std::printf("], \"length\": [");
    for (int k = 0; k < N_KINDS; ++k) std::printf("%s%lld", k ? ", " : "", status == SCAN_OK ? sc.length[k] : 0LL);
    std::printf("]");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, path;
        in >> cmd;
        if (cmd == "scan") {
            long long fluid_end = 0;
            in >> fluid_end >> path;
            std::FILE* f = std::fopen(path.c_str(), "rb");
            if (!f) {
                std::printf("{\"error\": \"cannot open\"}\n");
                continue;
            }
            Scan sc;
            const int st = scan(f, fluid_end, &sc);
            std::fclose(f);
            std::printf("{");
            print_scan(st, sc);
            std::printf("}\n");
        } else if (cmd == "info") {
            in >> path;
            std::FILE* f = std::fopen(path.c_str(), "rb");
            if (!f) {
                std::printf("{\"error\": \"cannot open\"}\n");
                continue;
            }
            long long iv[CK_NI];
            double dv[CK_ND];
            const long long fluid = read_fluid_header(f, iv, dv);
            std::printf("{\"fluid\": %lld, \"step\": %lld", fluid, fluid >= 0 ? iv[CK_T] : -1LL);
            if (fluid >= 0) {
                Scan sc;
                const int st = scan(f, fluid, &sc);
                std::printf(", ");
                print_scan(st, sc);
            }
            std::fclose(f);
            std::printf("}\n");
        } else {
            std::printf("{\"error\": \"unknown command\"}\n");
        }
    }
    return 0;
}
