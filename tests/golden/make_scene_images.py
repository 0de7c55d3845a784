#!/usr/bin/env python
"""Writes tests/golden/scene_images.npz: seeded field sets and every staging image that the pack_fields of commit REV -- the last one that
had it inside vfik_abi.cpp, with 14 output vectors -- made of them, in both I/O types, with that commit's per-arm results (slots, compact
slots, aux flag, pair state / safe / force, classify_arm's code).  tests/test_scene_plan.py holds vfik_scene.h's pack_fields to it byte for byte.

    python tests/golden/make_scene_images.py        (needs the git history and hipcc; no GPU)

The old function sits in an anonymous namespace of a file full of HIP calls: ADAPTER includes that file, calls nothing of HIP and is linked with
the launch entry points left unresolved.  It speaks tests/c_host/scene_plan.cpp's `pack` request and answer."""
import os
import subprocess
import tempfile

import numpy as np

REV = "cdee413"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIELD = np.dtype([("id", "<i4"), ("type", "<i4"), ("force", "<f8"), ("p", "<f8", (17,))])
IMAGES = ("goal", "aux", "slots", "compact", "uni", "orders", "repmap", "scenemaps")
SOURCES = ("vfclik_amd/csrc/vfik_abi.cpp", "vfclik_amd/csrc/vfik_kernel.h", "vfclik_amd/csrc/vfik_io_layout.h", "include/vfik.h", "include/vfik_types.h")

ADAPTER = r"""
#include "vfclik_amd/csrc/vfik_abi.cpp"
#include <iostream>
#include <sstream>
static std::vector<unsigned char> unhex(const std::string& s) {
    std::vector<unsigned char> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (unsigned char)std::strtol(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}
template <typename V> static void hex_line(const char* name, const V& v) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    std::printf("%s ", name);
    for (size_t i = 0; i < v.size() * sizeof(v[0]); ++i) std::printf("%02x", p[i]);
    std::printf("\n");
}
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string tok, fh, ch;
        int io = 32, S = 16, n_arms = 1, max_fields = 0;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
            if (k == "io") io = std::atoi(v.c_str());
            else if (k == "S") S = std::atoi(v.c_str());
            else if (k == "n_arms") n_arms = std::atoi(v.c_str());
            else if (k == "max_fields") max_fields = std::atoi(v.c_str());
            else if (k == "counts") ch = v;
            else if (k == "fields") fh = v;
        }
        auto cb = unhex(ch), fb = unhex(fh);
        std::vector<int32_t> counts(cb.size() / 4);
        std::memcpy(counts.data(), cb.data(), cb.size());
        std::vector<vfik_field> fields(fb.size() / sizeof(vfik_field) + 1);
        std::memcpy(fields.data(), fb.data(), fb.size());
        std::vector<char> goal, slots, fast, funnel, hasf(n_arms), uni, pstate(n_arms);
        std::vector<double> psafe(n_arms), pforce(n_arms);
        std::vector<int> used(n_arms), used_fast(n_arms);
        std::vector<unsigned char> ord;
        std::vector<unsigned short> rmap, smap;
        if (io == 32) pack_fields<float>(fields.data(), max_fields, counts.data(), n_arms, S, goal, slots, fast, used, funnel, used_fast, hasf, uni, pstate, psafe, pforce, ord, rmap, smap);
        else pack_fields<double>(fields.data(), max_fields, counts.data(), n_arms, S, goal, slots, fast, used, funnel, used_fast, hasf, uni, pstate, psafe, pforce, ord, rmap, smap);
        hex_line("goal", goal); hex_line("aux", funnel); hex_line("slots", slots); hex_line("compact", fast);
        hex_line("uni", uni); hex_line("orders", ord); hex_line("repmap", rmap); hex_line("scenemaps", smap);
        std::printf("arms");
        for (int j = 0; j < n_arms; ++j)
            std::printf(" %d,%d,%d,%d,%.17g,%.17g,%d", used[j], used_fast[j], (int)hasf[j], (int)pstate[j], psafe[j], pforce[j],
                        classify_arm(fields.data() + (size_t)j * max_fields, counts[j]));
        std::printf("\n");
    }
    return 0;
}
"""

SLOTS = {0: 0, 1: 3, 2: 1, 4: 2, 5: 2}   # device slots by field type (the first attractor is free)
N_PARAMS = {0: 0, 1: 17, 2: 6, 4: 8, 5: 10}


def scenes():
    """Two dozen field sets: at most 5 arms, max_slots 0 ... 8, at most 10 fields an arm, every type, shuffled ids, NULL fields, empty arms.
    Most numbers are multiples of 1/256 (the archive stays small), every tenth has all its bits (float32 rounds it)."""
    rng = np.random.default_rng(20261019)
    out = []
    for i in range(24):
        S = (0, 1, 2, 3, 5, 7, 8, 8)[i % 8]
        n_arms = int(rng.integers(1, 6))
        max_fields = int(rng.integers(6, 11))
        f = np.zeros((n_arms, max_fields), dtype=FIELD)
        counts = np.zeros(n_arms, dtype=np.int32)
        for j in range(n_arms):
            if rng.random() < 0.15:
                continue   # an arm without fields
            left, have_goal, k = S, False, 0
            ids = rng.permutation(40)[:max_fields] + (0 if rng.random() < 0.5 else -20)   # shuffled, some negative; a few equal ones below
            style = (0, 1, 1, 2, 3)[rng.integers(0, 5)]  # 0: the feeder's scene, 1: mixed integer orders, 2: any order, 3: any pair
            while k < max_fields and rng.random() < 0.9:
                t = int(rng.choice([0, 1, 2, 2, 2, 2, 2, 2, 4, 5]))
                need = 0 if (t == 1 and not have_goal) else SLOTS[t]
                if need > left:
                    if left == 0 and rng.random() < 0.6:
                        break
                    t, need = (2, 1) if left >= 1 else (0, 0)
                have_goal |= t == 1
                left -= need
                fd = f[j, k]
                fd["id"] = ids[k] if rng.random() < 0.9 else ids[0]
                fd["type"] = t
                fd["force"] = (1.0 if t in (1, 5) else -10.0) if style < 3 or rng.random() < 0.5 else rng.integers(-2560, 2560) / 256
                p = rng.integers(-256, 256, N_PARAMS[t]) / 256.0
                full = rng.random(N_PARAMS[t]) < 0.1
                p[full] = rng.uniform(-1, 1, int(full.sum()))
                if t == 2:
                    p[3] = abs(p[3])
                    p[4] = 0.001 if style < 3 or rng.random() < 0.5 else rng.choice([0.002, -2.0, 0.001 + 1e-12])
                    p[5] = 5.0 if style == 0 else rng.choice([5.0, 4.0, 20.0, 0.0] if style == 1 else [5.0, 2.5, 127.0, 128.0, -1.0, float("nan")])
                if t == 4:
                    p[7] = rng.choice([5.0, 5.0, 3.0, 1.5])
                if t == 5:
                    p[7], p[9] = rng.choice([10.0, 10.0, 130.0]), rng.choice([2.0, 2.0, 0.5])
                fd["p"][:N_PARAMS[t]] = p
                k += 1
            counts[j] = k
        out.append((S, f, counts))
    return out


def request(io, S, f, counts):
    return "io=%d S=%d n_arms=%d max_fields=%d counts=%s fields=%s" % (io, S, f.shape[0], f.shape[1], counts.tobytes().hex(), f.tobytes().hex())


def answers(exe, requests):
    """[{image: uint8 array, ..., "arms": float64 [n_arms][...]}] of a driver that speaks scene_plan.cpp's `pack`"""
    r = subprocess.run(exe, input="\n".join(requests) + "\n", capture_output=True, text=True, check=True, timeout=120)
    out, cur = [], {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name == "arms":
            cur["arms"] = np.array([[float(v) for v in a.split(",")] for a in rest.split()], dtype=np.float64)
            out.append(cur)
            cur = {}
        else:
            cur[name] = np.frombuffer(bytes.fromhex(rest), dtype=np.uint8)
    return out


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        for s in SOURCES:
            os.makedirs(os.path.dirname(os.path.join(d, s)), exist_ok=True)
            with open(os.path.join(d, s), "wb") as f:
                f.write(subprocess.check_output(["git", "-C", ROOT, "show", "%s:%s" % (REV, s)]))
        with open(os.path.join(d, "adapter.cpp"), "w") as f:
            f.write(ADAPTER)
        exe = os.path.join(d, "adapter")
        subprocess.check_call([hipcc, "-std=c++17", "-O1", "-w", "adapter.cpp", "-Wl,--unresolved-symbols=ignore-all", "-o", exe], cwd=d)
        sc = scenes()
        # few members (each costs the archive a header): per I/O type every image of every scene in one run of bytes with their lengths
        # [scene][image], the arms' results row after row; the field sets likewise, with [scene] = (max_slots, arms, max_fields)
        arrays = {"rev": np.array(REV), "shapes": np.array([(S, f.shape[0], f.shape[1]) for S, f, c in sc], dtype=np.int32),
                  "fields": np.concatenate([f.ravel() for S, f, c in sc]), "counts": np.concatenate([c for S, f, c in sc])}
        for io in (32, 64):
            got = answers([exe], [request(io, S, f, c) for S, f, c in sc])
            assert len(got) == len(sc)
            arrays["images%d" % io] = np.concatenate([g[name] for g in got for name in IMAGES])
            arrays["lengths%d" % io] = np.array([[len(g[name]) for name in IMAGES] for g in got], dtype=np.int32)
            arrays["arms%d" % io] = np.concatenate([g["arms"] for g in got])
    path = os.path.join(ROOT, "tests", "golden", "scene_images.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d scenes, %d bytes" % (path, len(sc), os.path.getsize(path)))


if __name__ == "__main__":
    main()
