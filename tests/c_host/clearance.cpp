// The clearance's argument checks and pair mask (vfclik_amd/csrc/vfik_links.h: clear_check, clear_mask) on the CPU: host code only, no GPU, no
// HIP header, no library -- built and run by tests/test_clearance_host.py, once plain and once with -fsanitize=address,undefined.  One request
// per line on stdin:
//   chain=<vfik_chain as hex> spheres=<L vfik_link_sphere as hex, or `none`> q=<0|1> pts=<address, decimal> clear=<0|1> n_rep= first= count=
//   mask=<L uint32 as hex, or `null`>
// q and clear say whether the pointer is given; pts is the address itself (only NULL and the alignment are looked at, nothing is read through it).
// The mask is copied into a heap block of exactly L words, so that a read past the caller's list is a finding of the sanitizer.  One answer per
// line:
//   rc=0 mask=<16 uint32 as hex: the mask in the image's sorted order>          or          rc=<-1|-4> msg=<clear_check's reason>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

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
        std::string tok, sph, msk;
        vfik_chain chain;
        int n_rep = 0, first = 0, count = 0, have = 0, has_q = 0, has_clear = 0;
        unsigned long long pts = 0;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            if (k == "chain" && unhex(v, &chain, sizeof chain)) have |= 1;
            else if (k == "spheres") { sph = v; have |= 2; }
            else if (k == "q") { has_q = std::atoi(v.c_str()); have |= 4; }
            else if (k == "pts") { pts = std::strtoull(v.c_str(), nullptr, 10); have |= 8; }
            else if (k == "clear") { has_clear = std::atoi(v.c_str()); have |= 16; }
            else if (k == "n_rep") { n_rep = std::atoi(v.c_str()); have |= 32; }
            else if (k == "first") { first = std::atoi(v.c_str()); have |= 64; }
            else if (k == "count") { count = std::atoi(v.c_str()); have |= 128; }
            else if (k == "mask") { msk = v; have |= 256; }
        }
        if (have != 511) {
            std::fprintf(stderr, "clearance: a request needs chain= spheres= q= pts= clear= n_rep= first= count= mask=\n");
            return 2;
        }
        const int L = sph == "none" ? 0 : (int)(sph.size() / (2 * sizeof(vfik_link_sphere)));
        vfik_link_sphere* list = static_cast<vfik_link_sphere*>(std::malloc(L ? L * sizeof(vfik_link_sphere) : 1));
        if (L && !unhex(sph, list, L * sizeof(vfik_link_sphere))) {
            std::fprintf(stderr, "clearance: spheres= is no whole number of vfik_link_sphere\n");
            return 2;
        }
        uint32_t* mask = nullptr;
        if (msk != "null") {
            mask = static_cast<uint32_t*>(std::malloc(L ? L * sizeof(uint32_t) : 1));
            if (!unhex(msk, mask, L * sizeof(uint32_t))) {
                std::fprintf(stderr, "clearance: mask= is not L words\n");
                return 2;
            }
        }
        char msg[160] = "";
        static const char some = 0;
        int rc = vfik::links_check(chain, list, L, msg, sizeof msg);
        if (rc == 0)
            rc = vfik::clear_check(L, has_q ? &some : nullptr, reinterpret_cast<const void*>((uintptr_t)pts), has_clear ? &some : nullptr, n_rep, first,
                                   count, mask, msg, sizeof msg);
        if (rc != 0) {
            std::printf("rc=%d msg=%s\n", rc, msg);
        } else {
            vfik::LinkImage img;
            vfik::links_fill(chain, list, L, &img);
            uint32_t sorted[VFIK_MAX_LINK_SPHERES];
            vfik::clear_mask(img, mask, count, sorted);
            std::printf("rc=0 mask=");
            const unsigned char* p = reinterpret_cast<const unsigned char*>(sorted);
            for (size_t i = 0; i < sizeof sorted; ++i) std::printf("%02x", p[i]);
            std::printf("\n");
        }
        std::free(mask);
        std::free(list);
    }
    return 0;
}
