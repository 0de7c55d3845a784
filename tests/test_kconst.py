"""A chain's device constants as pure host code (vfclik_amd/csrc/vfik_kconst.h: kconst_fill) on the CPU: tests/c_host/kconst.cpp -- built with
hipcc as plain C++, no HIP header, no GPU, no library -- turns a vfik_chain, vfik_params and a shared tool into the image the kernels read, the
`plain` code and the DH-pattern decision.

THE GOLDEN: tests/golden/kconst_images.npz holds two dozen requests (the three robots; five LWR variants one link off the pattern; a chain with
a prismatic joint and one with a trailing z-screw, from KDL-style segments; shared tools and IK weights for every `plain` code; tool blocks at
the rule's edge, past it and without an inverse; a base frame; rot_slowdown 0, inside (0, pi), pi and beyond; a frame that is no rigid motion;
a joint count that is not built) and what the kconst_fill of commit 0b8cd55 -- the last one that had it at the bottom of vfik_kernel.hip --
answered.  tests/golden/make_kconst_images.py wrote it and asserted there, on one machine with one libm, that this header answers with the
same bytes.  Here, on whatever libm the test machine has:
  * `plain`, `dhp` and every member that is a copy, plain IEEE arithmetic or a snapped value (the exact zeros and ones of a, d, ca, sa, an
    offset at a multiple of pi) equal the golden EXACTLY;
  * the members that come out of cos / sin / atan2 / sqrt agree to 1e-13 relative (absolute where the golden value is 0): a member is a
    handful of libm calls deep at 1 ulp each at most, and 1e-13 is four orders inside the library's own 1e-9 recomposition bar.

THE KINEMATICS: forward kinematics recomposed from the image -- base . prod_i Screw_z(q_i + off_i, d_i) Tx(a_i) Rx(alpha_i) . tail, with the
prismatic blends as KConst's comment states them -- equal Chain.fk(q) to 1e-12 at 16 seeded q per chain: rounding over at most 14 links of
at most 1 m is ~1e-14.  The parent's golden images are held to the same bound."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from vfclik_amd.chain import Chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_JOINTS, MIX = 16, 6
CHAIN = np.dtype([("n", "<i4"), ("jtype", "<i4", (MAX_JOINTS,)), ("pad", "<i4"), ("B", "<f8", (MAX_JOINTS + 1, 12)), ("q_lo", "<f8", (MAX_JOINTS,)),
                  ("q_hi", "<f8", (MAX_JOINTS,))])   # vfik_chain (include/vfik_types.h)
BUILT = (6, 7, 10, 14)   # VFIK_NJ_LIST
# DhPattern<n, 1> (vfik_kconst.h): SWAP, NONE, D0, OFF0, OFFPI; all three want the identity base
PATTERN = {7: (0x3F, 0x40, 0x2A, 0x15, 0x6A), 14: (0x1FBF, 0x2040, 0x152A, 0xA95, 0x356A), 6: (0x1D, 0x20, 0x16, 0x27, 0x18)}
# members that come out of libm calls (dh: off cprs sprs d a ca sa); every other byte of the image is a copy, IEEE arithmetic or long double arithmetic
LIBM_DH = ("off", "cprs", "sprs", "d", "a", "ca", "sa")
LIBM = ("tail_c", "tail_s", "tail_e", "cos_slow")
RTOL = 1e-13
FK_TOL = 1e-12


def kconst_dtype(nj):
    """KConst<nj> (vfik_kconst.h), then zeros up to a multiple of 1 KiB, then the 1-KiB (sin, cos)(k pi / 32) table"""
    dh = np.dtype([(k, "<f8") for k in ("off", "crev", "cprs", "sprs", "qd", "d", "a", "ca", "sa", "pad")])
    m = [("base", "<f8", (12,)), ("dh", dh, (nj,))] + [(k, "<f8") for k in (
        "tail_c", "tail_s", "tail_e", "rep_safe", "speed", "lambda2", "rot_slow", "null_gain", "lookahead", "max_vel", "cos_slow", "jp_kp", "jp_delta", "jl_gain")]
    m += [("mix_w", "<f8", (MIX,)), ("tool", "<f8", (12,)), ("wy", "<f8", (6,))]
    m += [(k, "<f8", (nj,)) for k in ("wq", "q_lo", "q_hi", "q_mid", "inv_half", "jl_k")] + [("prismatic_mask", "<u4"), ("pad0", "<u4")]
    size = np.dtype(m).itemsize
    return np.dtype(m + [("fill", "u1", ((size + 1023) // 1024 * 1024 - size,)), ("table", "<f8", (64, 2))])


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "kconst_images.npz"))
    ends = np.cumsum(z["lengths"])
    g = {"names": [str(n) for n in z["names"]], "chains": z["chains"].view(CHAIN)[:, 0], "params": z["params"], "tools": z["tools"],
         "worst": z["worst"], "plain": z["plain"], "dhp": z["dhp"], "images": [z["images"][e - n:e] for e, n in zip(ends, z["lengths"])]}
    assert len(g["names"]) == 24 and str(z["rev"]) == "0b8cd55"
    return g


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("kconst") / "kconst")
    # -x c++: no HIP mode, so nothing of HIP is included behind the source's back
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c_host", "kconst.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def answers(driver, golden):
    lines = ["chain=%s params=%s tool12=%s" % (golden["chains"][i].tobytes().hex(), golden["params"][i].tobytes().hex(), golden["tools"][i].tobytes().hex())
             for i in range(len(golden["names"]))]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, check=True)
    out = []
    for ln in r.stdout.splitlines():
        kv = dict(t.split("=", 1) for t in ln.split())
        img = np.frombuffer(bytes.fromhex(kv["image"]), dtype=np.uint8)
        assert len(img) == int(kv["bytes"])
        out.append({"worst": float(kv["worst"]), "plain": int(kv["plain"]), "dhp": int(kv["dhp"]), "image": img})
    assert len(out) == len(lines)
    return out


def close(got, ref):
    """the bound on a member that comes out of libm: 1e-13 relative, absolute where the golden value is 0"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(got - ref) <= RTOL * np.where(ref == 0.0, 1.0, np.abs(ref))))


def snapped(name, ref):
    """where a libm member holds a value kconst_fill snapped to: the exact zeros and ones of a, d, ca, sa; an offset at a multiple of pi"""
    if name in ("a", "d", "ca", "sa"):
        return (ref == 0.0) | (ref == 1.0)
    if name == "off":
        return ref == np.rint(ref / math.pi) * math.pi
    return np.zeros(ref.shape, dtype=bool)


def test_every_request_is_answered_as_the_parent_answered_it(golden, answers):
    for i, name in enumerate(golden["names"]):
        got, ref_img, nj = answers[i], golden["images"][i], int(golden["chains"][i]["n"])
        assert (got["plain"], got["dhp"]) == (int(golden["plain"][i]), int(golden["dhp"][i])), name
        if nj not in BUILT:
            assert got["worst"] == golden["worst"][i] == 1e300 and len(got["image"]) == len(ref_img) == 0, name
            continue
        assert abs(got["worst"] - golden["worst"][i]) <= RTOL, name
        dt = kconst_dtype(nj)
        assert len(got["image"]) == len(ref_img) == dt.itemsize, name
        a, b = got["image"].view(dt)[0].copy(), ref_img.view(dt)[0].copy()
        for k in LIBM_DH:
            fixed = snapped(k, b["dh"][k])
            assert np.array_equal(a["dh"][k][fixed], b["dh"][k][fixed]), (name, k)
            assert close(a["dh"][k], b["dh"][k]), (name, k)
            a["dh"][k] = b["dh"][k]
        for k in LIBM + ("table",):
            assert close(a[k], b[k]), (name, k)
            a[k] = b[k]
        assert a.tobytes() == b.tobytes(), name    # everything else: the golden's bytes
        assert int(a["prismatic_mask"]) == sum(1 << j for j in range(nj) if golden["chains"][i]["jtype"][j] == 1), name


def test_plain_pattern_and_error_are_what_each_request_stands_for(golden, answers):
    got = {n: a for n, a in zip(golden["names"], answers)}
    code = lambda n: (got[n]["plain"], got[n]["dhp"])
    assert [code(n) for n in ("lwr", "lwr_dual14", "powercube6")] == [(1, 1)] * 3
    assert [got["lwr_variant%d" % k]["dhp"] for k in range(5)] == [0, 0, 0, 1, 0] and all(got["lwr_variant%d" % k]["plain"] == 1 for k in range(5))
    assert code("prismatic7") == (0, 0) and code("tail_screw7") == (0, 0)
    assert [code(n) for n in ("lwr", "lwr_tool", "lwr_weights", "lwr_joint_weights", "lwr_tool_weights")] == [(1, 1), (2, 1), (3, 1), (3, 1), (4, 1)]
    assert code("lwr_tool_shear_062") == (2, 1) and code("lwr_tool_shear_063") == (0, 0) and code("lwr_tool_flat") == (0, 0)
    assert code("lwr_on_a_base") == (1, 0)
    # the bar vfik_abi.cpp's upload_kconst applies: a chain whose frames recompose worse than 1e-9 is refused
    assert got["lwr_stretched_frame"]["worst"] >= 1e-9 and got["nine_joints_not_built"]["worst"] == 1e300
    assert all(a["worst"] < 1e-9 for n, a in got.items() if n not in ("lwr_stretched_frame", "nine_joints_not_built"))
    dt = kconst_dtype(7)
    image = lambda n: got[n]["image"].view(dt)[0]
    # cos_slow: cos(rot_slow) inside (0, pi), else -2 (always evaluate the angle); 1 / rot_slow in dh[1].pad, 0 without a slow-down
    for n, rs in (("rot_slow_0", 0.0), ("lwr", 0.3), ("rot_slow_1", 1.0), ("rot_slow_pi", math.pi), ("rot_slow_4", 4.0)):
        c = image(n)
        assert c["rot_slow"] == rs and c["dh"][1]["pad"] == (1.0 / rs if rs > 0.0 else 0.0), n
        assert (abs(c["cos_slow"] - math.cos(rs)) <= RTOL) if 0.0 < rs < math.pi else c["cos_slow"] == -2.0, n
    # the prismatic blends and the trailing screw are in the image
    c = image("prismatic7")
    assert int(c["prismatic_mask"]) == 4 and list(c["dh"]["crev"]) == [1, 1, 0, 1, 1, 1, 1] and list(c["dh"]["qd"]) == [0, 0, 1, 0, 0, 0, 0]
    c = image("tail_screw7")
    assert abs(c["tail_c"] - math.cos(0.4)) < 1e-12 and abs(c["tail_s"] - math.sin(0.4)) < 1e-12 and abs(c["tail_e"] - 0.05) < 1e-12


def masks_of(c, nj):
    """the masks kconst_fill_t hands dh_pattern_of, read back from an image"""
    swap = none = d0 = off0 = offpi = 0
    for i in range(nj):
        d = c["dh"][i]
        if d["crev"] != 1.0:
            continue
        swap |= int(d["a"] == 0.0 and d["ca"] == 0.0 and d["sa"] == 1.0) << i
        none |= int(d["a"] == 0.0 and d["ca"] == 1.0 and d["sa"] == 0.0) << i
        d0 |= int(d["d"] == 0.0) << i
        k = round(d["off"] / math.pi)
        if d["off"] == k * math.pi:
            off0 |= int(k % 2 == 0) << i
            offpi |= int(k % 2 == 1) << i
    return swap, none, d0, off0, offpi


def test_the_built_robots_masks_contain_their_pattern(golden, answers):
    for i, name in enumerate(golden["names"]):
        nj = int(golden["chains"][i]["n"])
        if nj not in BUILT or answers[i]["plain"] == 0:
            continue
        for img in (answers[i]["image"], golden["images"][i]):
            c = img.view(kconst_dtype(nj))[0]
            base_i = list(c["base"]) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
            contains = all((m & p) == p for m, p in zip(masks_of(c, nj), PATTERN[nj])) and base_i
            assert contains == bool(answers[i]["dhp"]), name
    assert all(answers[golden["names"].index(n)]["dhp"] == 1 for n in ("lwr", "lwr_dual14", "powercube6"))


def fk_from_image(c, nj, q):
    X = np.vstack([c["base"].reshape(3, 4), [0, 0, 0, 1]])
    for i in range(nj):
        d = c["dh"][i]
        cs = d["crev"] * math.cos(q[i] + d["off"]) + d["cprs"]
        sn = d["crev"] * math.sin(q[i] + d["off"]) + d["sprs"]
        screw = np.array([[cs, -sn, 0, 0], [sn, cs, 0, 0], [0, 0, 1, d["qd"] * q[i] + d["d"]], [0, 0, 0, 1]])
        link = np.array([[1, 0, 0, d["a"]], [0, d["ca"], -d["sa"], 0], [0, d["sa"], d["ca"], 0], [0, 0, 0, 1]])
        X = X @ screw @ link
    return X @ np.array([[c["tail_c"], -c["tail_s"], 0, 0], [c["tail_s"], c["tail_c"], 0, 0], [0, 0, 1, c["tail_e"]], [0, 0, 0, 1]])


def test_the_image_recomposes_the_chains_forward_kinematics(golden, answers):
    rng = np.random.default_rng(7)
    seen = 0
    for i, name in enumerate(golden["names"]):
        ch = golden["chains"][i]
        nj = int(ch["n"])
        if nj not in BUILT or golden["worst"][i] >= 1e-9:
            continue
        chain = Chain(ch["B"][:nj + 1], ch["jtype"][:nj], ch["q_lo"][:nj], ch["q_hi"][:nj])
        q = rng.uniform(chain.q_lo, chain.q_hi, (16, nj))
        ref = chain.fk(q)
        for which, img in (("driver", answers[i]["image"]), ("golden", golden["images"][i])):
            c = img.view(kconst_dtype(nj))[0]
            err = max(np.abs(fk_from_image(c, nj, q[b]) - ref[b]).max() for b in range(16))
            assert err <= FK_TOL, (name, which, err)
        seen += 1
    assert seen == 22
