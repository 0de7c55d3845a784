// The link spheres' checks and device image (vfclik_amd/csrc/vfik_links.h) on the CPU: host code only, no GPU, no HIP header, no library -- built
// and run by tests/test_links_host.py, once plain and once with -fsanitize=address,undefined.  One request per line on stdin:
//   chain=<vfik_chain as hex> L=<count> spheres=<L vfik_link_sphere as hex, or `null`>
// The list is copied into a heap block of exactly L entries, so that a read past the caller's list is a finding of the sanitizer.  One answer
// per line:
//   rc=0 image=<LinkImage as hex>          or          rc=-1 msg=<links_check's reason>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../vfclik_amd/csrc/vfik_links.h"

namespace {

bool unhex(const std::string& s, void* out, size_t bytes) {
    if (s.size() != 2 * bytes) return false;
    unsigned char* p = static_cast<unsigned char*>(out);
    for (size_t i = 0; i < bytes; ++i) p[i] = (unsigned char)std::strtol(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return true;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string tok, sph;
        vfik_chain chain;
        int L = 0, have = 0;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            if (k == "chain" && unhex(v, &chain, sizeof chain)) have |= 1;
            else if (k == "L") { L = std::atoi(v.c_str()); have |= 2; }
            else if (k == "spheres") { sph = v; have |= 4; }
        }
        if (have != 7) {
            std::fprintf(stderr, "links: a request needs chain=, L= and spheres=\n");
            return 2;
        }
        vfik_link_sphere* list = nullptr;
        if (sph != "null") {
            const size_t count = sph.size() / (2 * sizeof(vfik_link_sphere));
            list = static_cast<vfik_link_sphere*>(std::malloc(count ? count * sizeof(vfik_link_sphere) : 1));
            if (!unhex(sph, list, count * sizeof(vfik_link_sphere))) {
                std::fprintf(stderr, "links: spheres= is no whole number of vfik_link_sphere\n");
                return 2;
            }
        }
        char msg[160] = "";
        const int rc = vfik::links_check(chain, list, L, msg, sizeof msg);
        if (rc != 0) {
            std::printf("rc=%d msg=%s\n", rc, msg);
        } else {
            vfik::LinkImage img;
            vfik::links_fill(chain, list, L, &img);
            std::printf("rc=0 image=");
            const unsigned char* p = reinterpret_cast<const unsigned char*>(&img);
            for (size_t i = 0; i < sizeof img; ++i) std::printf("%02x", p[i]);
            std::printf("\n");
        }
        std::free(list);
    }
    return 0;
}
