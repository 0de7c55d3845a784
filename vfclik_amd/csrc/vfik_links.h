// vfik_links.h -- spheres fixed to links of the chain (vfik_set_link_spheres) and how the host derives what link_kernel reads: the checks of
// the caller's list, and links_fill: vfik_chain + the spheres -> LinkImage, a small block in device memory that the kernel reads at
// wave-uniform addresses (scalar loads).  Pure host code on the C++ standard library and include/vfik_types.h: no HIP symbol, so a
// stand-alone program holds it on the CPU (tests/test_links_host.py).  The device code reads LinkImage through vfik_kernel.h, which includes
// this header; vfik_abi.cpp uploads the image.  Behind them, likewise pure host code: the argument checks of vfik_link_clearance and the
// pair mask in the image's order (clear_check, clear_mask; tests/test_clearance_host.py), and the checks of vfik_link_avoid and
// vfik_set_avoid_rule (avoid_check, avoid_rule_check; tests/test_avoid_host.py).
//
// Frames are those of the PUBLIC chain, X_link = B[0] Jz(q_1) B[1] ... Jz(q_link) B[link] (vfik_types.h).  The DH form of the cycle kernels
// (vfik_kconst.h: dh_factor) moves z-screws between neighbouring links -- its intermediate frames are not the caller's -- so KConst is of
// no use here and the image carries B[0..n] as they came.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include <stdint.h>

#include "../../include/vfik_types.h"

namespace vfik {

// The walk emits a sphere when it reaches the sphere's link, so the spheres are SORTED BY LINK (stable: spheres of one link keep the caller's
// order) and perm[] leads back: the sphere at sorted position i is the caller's sphere perm[i], and goes into the caller's row perm[i].
struct LinkImage {
    int32_t n, L;                              // joints, spheres
    int32_t jtype[VFIK_MAX_JOINTS];            // 0 revolute, 1 prismatic; entries from n on are 0
    int32_t link[VFIK_MAX_LINK_SPHERES];       // ascending; entries from L on are -1
    int32_t perm[VFIK_MAX_LINK_SPHERES];       // sorted position -> the caller's index; entries from L on are 0
    double B[VFIK_MAX_JOINTS + 1][12];         // row-major 3x4 [R | p]; entries beyond n are 0
    double c[VFIK_MAX_LINK_SPHERES][4];        // x y z radius, sorted; entries from L on are 0
};

// 0, or -1 (VFIK_E_ARG) with the reason in msg: L outside 0..16, a missing list, a link outside 0..n, a centre that is not finite, a radius
// that is negative or not finite, reserved != 0.
inline int links_check(const vfik_chain& ch, const vfik_link_sphere* s, int L, char* msg, size_t len) {
    if (L < 0 || L > VFIK_MAX_LINK_SPHERES) {
        std::snprintf(msg, len, "%d link spheres: 0..%d", L, VFIK_MAX_LINK_SPHERES);
        return -1;
    }
    if (L > 0 && !s) {
        std::snprintf(msg, len, "%d link spheres and no list", L);
        return -1;
    }
    for (int j = 0; j < L; ++j) {
        if (s[j].link < 0 || s[j].link > ch.n) {
            std::snprintf(msg, len, "link sphere %d: link %d outside 0..%d", j, s[j].link, ch.n);
            return -1;
        }
        if (s[j].reserved != 0) {
            std::snprintf(msg, len, "link sphere %d: reserved must be 0", j);
            return -1;
        }
        if (!std::isfinite(s[j].c[0]) || !std::isfinite(s[j].c[1]) || !std::isfinite(s[j].c[2])) {
            std::snprintf(msg, len, "link sphere %d: the centre is not finite", j);
            return -1;
        }
        if (!std::isfinite(s[j].radius) || s[j].radius < 0.0) {
            std::snprintf(msg, len, "link sphere %d: radius %g must be finite and not negative", j, s[j].radius);
            return -1;
        }
    }
    return 0;
}

// The image of a checked list (links_check returned 0).
inline void links_fill(const vfik_chain& ch, const vfik_link_sphere* s, int L, LinkImage* im) {
    std::memset(im, 0, sizeof *im);
    im->n = ch.n;
    im->L = L;
    for (int i = 0; i < ch.n; ++i) im->jtype[i] = ch.jtype[i];
    for (int i = 0; i <= ch.n; ++i) std::memcpy(im->B[i], ch.B[i], sizeof im->B[i]);
    for (int j = 0; j < VFIK_MAX_LINK_SPHERES; ++j) im->link[j] = -1;
    int at = 0;
    for (int l = 0; l <= ch.n; ++l)         // a counting sort by link: stable
        for (int j = 0; j < L; ++j) {
            if (s[j].link != l) continue;
            im->link[at] = l;
            im->perm[at] = j;
            im->c[at][0] = s[j].c[0]; im->c[at][1] = s[j].c[1]; im->c[at][2] = s[j].c[2];
            im->c[at][3] = s[j].radius;
            ++at;
        }
}

// ---- vfik_link_clearance / vfik_set_wait_rule: the checks of the caller's row window and pair mask, and the mask as clear_kernel reads it ----
// A pair mask is one word per OWN sphere in the caller's order: bit j of mask[i] lets own sphere i meet row first + j.  The kernel visits
// the own spheres in the image's sorted order, so the mask travels permuted: sorted[i] = mask[perm[i]].

// 0, -1 (VFIK_E_ARG) or -4 (VFIK_E_STATE: no spheres set) with the reason in msg.  L own spheres; rows first .. first + count - 1 of n_rep;
// q, pts4, clear as the caller gave them (only NULL and pts4's alignment are looked at); mask: L words or NULL (every pair).
inline int clear_check(int L, const void* q, const void* pts4, const void* clear, int n_rep, int first, int count, const uint32_t* mask, char* msg,
                       size_t len) {
    if (!q || !pts4 || !clear) {
        std::snprintf(msg, len, "q, pts4 and clear are required");
        return -1;
    }
    if (reinterpret_cast<uintptr_t>(pts4) % 16) {
        std::snprintf(msg, len, "pts4 must be 16-byte aligned: the kernel loads its rows in 16-byte pieces");
        return -1;
    }
    if (count < 1 || count > 32) {
        std::snprintf(msg, len, "count %d outside 1..32", count);
        return -1;
    }
    if (first < 0 || n_rep < 0 || first > n_rep - count) {
        std::snprintf(msg, len, "rows [%d, %d + %d) outside the %d rows of pts4", first, first, count, n_rep);
        return -1;
    }
    if (L < 1) {
        std::snprintf(msg, len, "no link spheres set: there is nothing to measure from");
        return -4;
    }
    if (L > VFIK_MAX_LINK_SPHERES) {
        std::snprintf(msg, len, "%d link spheres: 1..%d", L, VFIK_MAX_LINK_SPHERES);
        return -1;
    }
    for (int i = 0; mask && i < L; ++i)
        if (count < 32 && (mask[i] >> count) != 0) {
            std::snprintf(msg, len, "mask[%d] = 0x%08x names a row at or beyond count %d", i, (unsigned)mask[i], count);
            return -1;
        }
    return 0;
}

// The mask of a checked request in the image's order: sorted[i] = mask[perm[i]], every one of the `count` rows where mask is NULL; words
// from L on are 0.
inline void clear_mask(const LinkImage& im, const uint32_t* mask, int count, uint32_t sorted[VFIK_MAX_LINK_SPHERES]) {
    const uint32_t all = count >= 32 ? 0xFFFFFFFFu : ((1u << count) - 1u);
    for (int i = 0; i < VFIK_MAX_LINK_SPHERES; ++i) sorted[i] = i < im.L ? (mask ? mask[im.perm[i]] : all) : 0u;
}

// ---- vfik_link_avoid / vfik_set_avoid_rule: the checks of a push (avoid_kernel) ----
// The law's own parameters, shared by the call and the rule.  0 or -1 with the reason in msg.
inline int avoid_law_check(double gain, double d0, char* msg, size_t len) {
    if (!std::isfinite(d0) || !(d0 > 0.0)) {
        std::snprintf(msg, len, "d0 = %g: the influence distance must be finite and greater than 0", d0);
        return -1;
    }
    if (!std::isfinite(gain)) {
        std::snprintf(msg, len, "gain = %g must be finite", gain);
        return -1;
    }
    return 0;
}

// A mixer channel that a push may write: 3..5 (2 is the joint controller's).  `none_ok`: -1, no channel, passes.
inline int avoid_channel_check(int channel, bool none_ok, char* msg, size_t len) {
    if (none_ok && channel == -1) return 0;
    if (channel == 2) {
        std::snprintf(msg, len, "channel 2 is the joint controller's: 3..%d take a push", VFIK_MIX_CHANNELS - 1);
        return -1;
    }
    if (channel < 3 || channel >= VFIK_MIX_CHANNELS) {
        std::snprintf(msg, len, none_ok ? "channel %d: -1 (none) or 3..%d" : "channel %d outside 3..%d", channel, VFIK_MIX_CHANNELS - 1);
        return -1;
    }
    return 0;
}

// vfik_link_avoid: 0, -1 (VFIK_E_ARG) or -4 (VFIK_E_STATE: no spheres set; a channel and no ext buffer) with the reason in msg.  The row window
// and the mask are clear_check's (its `clear` stands for "some destination": out, or a channel); then the law and the channel.
inline int avoid_check(int L, const void* q, const void* pts4, const void* out, int n_rep, int first, int count, const uint32_t* mask, double gain,
                       double d0, int channel, bool have_ext, char* msg, size_t len) {
    if (avoid_channel_check(channel, true, msg, len) != 0) return -1;
    if (!out && channel < 0) {
        std::snprintf(msg, len, "out is required where no channel takes the command");
        return -1;
    }
    const int rc = clear_check(L, q, pts4, q /* a destination exists */, n_rep, first, count, mask, msg, len);
    if (rc != 0) return rc;
    if (avoid_law_check(gain, d0, msg, len) != 0) return -1;
    if (channel >= 0 && !have_ext) {
        std::snprintf(msg, len, "channel %d: the handle has no ext buffer yet (vfik_set_ext_cmd or vfik_set_avoid_rule allocates it)", channel);
        return -4;
    }
    return 0;
}

// vfik_set_avoid_rule: the rule's numbers (the pointers are the library's to look at).  L own spheres against the partner's L.
inline int avoid_rule_check(int L, double gain, double d0, int channel, int reserved, const uint32_t mask[VFIK_MAX_LINK_SPHERES], char* msg, size_t len) {
    if (avoid_law_check(gain, d0, msg, len) != 0) return -1;
    if (avoid_channel_check(channel, false, msg, len) != 0) return -1;
    if (reserved != 0) {
        std::snprintf(msg, len, "reserved must be 0");
        return -1;
    }
    for (int i = 0; i < VFIK_MAX_LINK_SPHERES; ++i)
        if ((i >= L && mask[i] != 0) || (L < 32 && (mask[i] >> L) != 0)) {
            std::snprintf(msg, len, "mask[%d] = 0x%08x names a sphere at or beyond the %d of the handle", i, (unsigned)mask[i], L);
            return -1;
        }
    return 0;
}

}  // namespace vfik
