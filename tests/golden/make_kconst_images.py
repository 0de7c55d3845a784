#!/usr/bin/env python
"""Writes tests/golden/kconst_images.npz: two dozen chains with parameters and a shared tool, and what the kconst_fill of commit REV -- the last
one that had it behind `#else // VFIK_DISPATCH` at the bottom of vfik_kernel.hip -- made of them: the whole image of the device constants,
`plain`, `dhp`, the recomposition error.  tests/test_kconst.py holds vfclik_amd/csrc/vfik_kconst.h to it.

    python tests/golden/make_kconst_images.py        (needs the git history and hipcc; no GPU)

The old functions sit in a file of device code: the adapter is tests/c_host/kconst.cpp's main() behind that commit's vfik_kernel.hip instead of
vfik_kconst.h, compiled as HIP host code only with -DVFIK_DISPATCH; it calls nothing of HIP and is linked with the per-part launch entry points
left unresolved.  Before it writes the archive this script builds today's driver too and asserts that both answer every request with the same
BYTES (same machine, same libm); the test allows the transcendental members the last bits of another libm."""
import ctypes
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

REV = "0b8cd55"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vfclik_amd import _abi, robots  # noqa: E402
from vfclik_amd.chain import PRISMATIC, REVOLUTE, Chain, _hom, _rot_x, _rot_z  # noqa: E402

SOURCES = ("vfclik_amd/csrc/vfik_kernel.hip", "vfclik_amd/csrc/vfik_kernel.h", "vfclik_amd/csrc/vfik_check_body.inc", "include/vfik.h", "include/vfik_types.h")
DRIVER = os.path.join(ROOT, "tests", "c_host", "kconst.cpp")
DRIVER_INCLUDE = '#include "../../vfclik_amd/csrc/vfik_kconst.h"\n'
IDENT = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
TOOL = (1, 0, 0, 0.02, 0, 1, 0, -0.01, 0, 0, 1, 0.2)   # a hand: the identity block and an offset
LWR_VARIANTS = ((2, (0.05, -math.pi / 2, 0.4, 0.0), 0),    # tests/test_gpu_dh_pattern.py, test_chains_that_do_not_match...: a != 0
                (3, (0.0, 1.0, 0.0, 0.0), 0),              # alpha = 1 rad
                (1, (0.0, -math.pi / 2, 0.02, 0.0), 0),    # d != 0 where the pattern has d = 0
                (0, (0.0, math.pi / 2, 0.0, 0.0), 1),      # one more zero: still the pattern
                (6, (0.0, math.pi / 2, 0.078, 0.0), 0))    # the last link twisted


def requests():
    """[(name, Chain, Params, tool12, expected plain or None, expected dhp or None)]"""
    lim = np.array(robots._LWR_LIM)
    lwr = robots.lwr()
    P = _abi.default_params
    out = [("lwr", lwr, P(), IDENT, 1, 1), ("lwr_dual14", robots.lwr_dual14(), P(flags=7, jl_gain=0.25), IDENT, 1, 1),
           ("powercube6", robots.powercube6(), P(flags=5), IDENT, 1, 1)]
    for k, (row, dh_row, expect) in enumerate(LWR_VARIANTS):
        dh = list(robots._LWR_DH)
        dh[row] = dh_row
        out.append(("lwr_variant%d" % k, Chain.from_dh(dh, -lim, lim), P(flags=5), IDENT, 1, expect))
    # KDL-style segments: joint axes off z, tip frames with all their bits; the third joint slides
    rng = np.random.default_rng(20261020)

    def tip():
        return _hom(_rot_z(rng.uniform(-1, 1)) @ _rot_x(rng.uniform(-2, 2)) @ _rot_z(rng.uniform(-1, 1)), rng.uniform(-0.3, 0.3, 3))
    axes = [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 0), (0.6, 0, 0.8), (0, 0, 1), (1, 1, 0)]
    seg = [(PRISMATIC if i == 2 else REVOLUTE, axes[i], tip()) for i in range(7)]
    lo = np.array([-2.9, -2.0, -0.2, -2.0, -2.9, -2.0, -2.9])
    out.append(("prismatic7", Chain.from_segments(seg, lo, -lo), P(), IDENT, 0, 0))
    # the LWR's joints as segments about z, the last tip frame ending in a z-screw that no joint behind it absorbs
    seg = [(REVOLUTE, (0, 0, 1), _hom(None, [0, 0, d]) @ _hom(_rot_x(al))) for (a, al, d, off) in robots._LWR_DH[:6]]
    seg.append((REVOLUTE, (0, 0, 1), _hom(_rot_x(math.pi / 2)) @ _hom(_rot_z(0.4), [0, 0, 0.05])))
    out.append(("tail_screw7", Chain.from_segments(seg, -lim, lim), P(), IDENT, 0, 0))
    wy, wq = (1, 1, 1, 0.5, 0.5, 0.5), (1, 1, 2, 1, 1, 1, 0.25) + (1,) * 9
    out += [("lwr_tool", lwr, P(), TOOL, 2, 1), ("lwr_weights", lwr, P(wy=wy), IDENT, 3, 1), ("lwr_joint_weights", lwr, P(wq=wq), IDENT, 3, 1),
            ("lwr_tool_weights", lwr, P(wy=wy, wq=wq), TOOL, 4, 1)]
    shear = list(TOOL)
    shear[1] = 0.062     # max |R R^T - I| = 0.062 <= VFIK_TOOL_MAX_DEFECT: still a plain + tool handle
    out.append(("lwr_tool_shear_062", lwr, P(), tuple(shear), 2, 1))
    shear[1] = 0.063     # refused
    out.append(("lwr_tool_shear_063", lwr, P(), tuple(shear), 0, 0))
    flat = list(TOOL)
    flat[2] = flat[6] = flat[10] = 0.0   # no inverse
    out.append(("lwr_tool_flat", lwr, P(), tuple(flat), 0, 0))
    base = _hom(_rot_z(0.3) @ _rot_x(-0.2), [0.1, -0.2, 0.7])
    out.append(("lwr_on_a_base", Chain.from_dh(robots._LWR_DH, -lim, lim, base=base), P(), IDENT, 1, 0))
    for name, rs in (("rot_slow_0", 0.0), ("rot_slow_1", 1.0), ("rot_slow_pi", math.pi), ("rot_slow_4", 4.0)):
        out.append((name, lwr, P(rot_slowdown=rs), IDENT, 1, 1))
    B = lwr.B.copy()
    B[3, :, :3] *= 1.001     # not a rigid motion: the recomposition error says so
    out.append(("lwr_stretched_frame", Chain(B, lwr.jtype, lwr.q_lo, lwr.q_hi), P(), IDENT, None, None))
    nine = list(robots._LWR_DH) + list(robots._LWR_DH[:2])
    out.append(("nine_joints_not_built", Chain.from_dh(nine, -np.ones(9), np.ones(9)), P(), IDENT, None, None))
    return out


def line(chain, params, tool12):
    return "chain=%s params=%s tool12=%s" % (bytes(chain.to_struct()).hex(), bytes(params).hex(), np.asarray(tool12, dtype="<f8").tobytes().hex())


def answers(exe, lines):
    """[(worst, plain, dhp, image bytes)] of a driver that speaks tests/c_host/kconst.cpp's protocol"""
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=120)
    out = []
    for ln in r.stdout.splitlines():
        kv = dict(t.split("=", 1) for t in ln.split())
        img = np.frombuffer(bytes.fromhex(kv["image"]), dtype=np.uint8)
        assert len(img) == int(kv["bytes"])
        out.append((float(kv["worst"]), int(kv["plain"]), int(kv["dhp"]), img))
    return out


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    reqs = requests()
    lines = [line(c, p, t) for _, c, p, t, _, _ in reqs]
    with tempfile.TemporaryDirectory() as d:
        for s in SOURCES:
            os.makedirs(os.path.dirname(os.path.join(d, s)), exist_ok=True)
            with open(os.path.join(d, s), "wb") as f:
                f.write(subprocess.check_output(["git", "-C", ROOT, "show", "%s:%s" % (REV, s)]))
        main_text = open(DRIVER).read()
        assert main_text.count(DRIVER_INCLUDE) == 1
        with open(os.path.join(d, "adapter.hip"), "w") as f:
            f.write('#include "vfclik_amd/csrc/vfik_kernel.hip"\n' + main_text.replace(DRIVER_INCLUDE, ""))
        subprocess.check_call([hipcc, "-std=c++17", "-O1", "-w", "-DVFIK_DISPATCH", "--offload-arch=gfx950", "--cuda-host-only", "adapter.hip",
                               "-Wl,--unresolved-symbols=ignore-all", "-o", "adapter"], cwd=d)
        subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", DRIVER, "-o", os.path.join(d, "kconst")])
        old, new = answers(os.path.join(d, "adapter"), lines), answers(os.path.join(d, "kconst"), lines)
    assert len(old) == len(new) == len(reqs)
    for (name, _, _, _, plain, dhp), (w0, p0, d0, i0), (w1, p1, d1, i1) in zip(reqs, old, new):
        assert (np.float64(w0).tobytes(), p0, d0, i0.tobytes()) == (np.float64(w1).tobytes(), p1, d1, i1.tobytes()), name
        assert plain is None or (p0, d0) == (plain, dhp), (name, p0, d0)
    arrays = {"rev": np.array(REV), "names": np.array([r[0] for r in reqs]),
              "chains": np.stack([np.frombuffer(bytes(r[1].to_struct()), dtype=np.uint8) for r in reqs]),
              "params": np.stack([np.frombuffer(bytes(r[2]), dtype=np.uint8) for r in reqs]),
              "tools": np.array([r[3] for r in reqs], dtype=np.float64),
              "worst": np.array([a[0] for a in old]), "plain": np.array([a[1] for a in old], dtype=np.int32), "dhp": np.array([a[2] for a in old], dtype=np.int32),
              "lengths": np.array([len(a[3]) for a in old], dtype=np.int32), "images": np.concatenate([a[3] for a in old])}
    assert ctypes.sizeof(_abi.Chain) == arrays["chains"].shape[1] and ctypes.sizeof(_abi.Params) == arrays["params"].shape[1]
    path = os.path.join(ROOT, "tests", "golden", "kconst_images.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d requests, %d bytes; vfik_kconst.h answers all %d with commit %s's bytes (image, plain, dhp, worst)" % (
        os.path.relpath(path, ROOT), len(reqs), os.path.getsize(path), len(reqs), REV))


if __name__ == "__main__":
    main()
