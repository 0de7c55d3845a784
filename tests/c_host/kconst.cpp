// A chain's device constants (vfclik_amd/csrc/vfik_kconst.h) on the CPU: host code only, no GPU, no HIP header, no library -- built and run by
// tests/test_kconst.py.  One request per line on stdin, `key=value` pairs; the structs of include/vfik_types.h travel as hex bytes:
//   chain=<vfik_chain> params=<vfik_params> tool12=<12 doubles: rows 0..2 of the shared tool>
// The joint count is the chain's n, as for a handle (vfik_abi.cpp: upload_kconst).  One answer per line:
//   worst=<kconst_fill's recomposition error, %.17g> plain=<0..4> dhp=<0|1> bytes=<kconst_bytes> image=<the whole image as hex>
// (a joint count that is not built: worst=1e+300, bytes=0 and an empty image).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../vfclik_amd/csrc/vfik_kconst.h"

namespace {

// the bytes of a plain struct from hex; false when the length is not the struct's
template <typename S>
bool unhex(const std::string& s, S* out) {
    if (s.size() != 2 * sizeof(S)) return false;
    unsigned char* p = reinterpret_cast<unsigned char*>(out);
    for (size_t i = 0; i < sizeof(S); ++i) p[i] = (unsigned char)std::strtol(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return true;
}

struct Tool { double v[12]; };

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string tok;
        vfik_chain chain;
        vfik_params params;
        Tool tool;
        int have = 0;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            if (k == "chain" && unhex(v, &chain)) have |= 1;
            else if (k == "params" && unhex(v, &params)) have |= 2;
            else if (k == "tool12" && unhex(v, &tool)) have |= 4;
        }
        if (have != 7 || chain.n < 1 || chain.n > VFIK_MAX_JOINTS) {
            std::fprintf(stderr, "kconst: a request needs chain=, params= and tool12= of the structs' sizes, and 1..%d joints\n", VFIK_MAX_JOINTS);
            return 2;
        }
        std::vector<unsigned char> img(vfik::kconst_bytes(chain.n));
        int plain = -1, dhp = -1;
        const double worst = vfik::kconst_fill(chain.n, img.data(), chain, params, tool.v, &plain, &dhp);
        std::printf("worst=%.17g plain=%d dhp=%d bytes=%zu image=", worst, plain, dhp, img.size());
        for (unsigned char b : img) std::printf("%02x", b);
        std::printf("\n");
    }
    return 0;
}
