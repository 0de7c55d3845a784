"""The C oracle and the NumPy restatement against the high-precision reference (tests/hp_reference.py) with a hand on the arm: the tool
pose T_tip = T_flange Tool (vf:321-332), Twist.RefPoint(p_ee - p_tip) (vf:456-459) and /pose_no_tool -- what the references of the
conditioning, field and nullspace sweeps leave out ("identity tool").

The tools are hp.TOOLS: rotations good to the last bit of a double, the same rotation as a float32 file or a hand-written config holds it
(3 x 3 blocks that are off a rotation by 5e-8 ... 9e-4), equal per-arm rows, per-arm tools, and a block without an inverse.  KDL's frame
product takes any nine numbers, and so does the reference: nothing here assumes Rtool^T = Rtool^-1.

Bars.  pose and pose_nt: 1e-14.  qdot_vf, per arm: err <= 8 unit, unit = cond u (max |qdot| + max |qdot_shift|), qdot_shift the solve of
(w x AB, 0) alone: w x AB can cancel v, and the rounding of either part stays.  R, the worst err / unit of a case, is printed: it is the
input of the GPU test's bar (tests/test_gpu_tool.py recomputes it from the same calls).

Measured on these cases (this file's own print, 108 cases with the two I/O types): the C oracle's worst R is 1.53 (lwr_dual14, float64,
lambda 0.1, `turned`), the NumPy restatement's 1.27; the worst pose error is 1.2e-15 (`long`).  The point shift reaches 13 times the
twist's own qdot (`per-arm`, lambda 1e-3)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_reference as hp  # noqa: E402

IO = [np.float32, np.float64]
POSE_BAR = 1e-14
K_ORACLE = 8.0
NP_ARMS = tuple(range(0, hp.B_ARMS, 17))    # the NumPy restatement is slow: 12 arms, every kind among them
CASES = [(robot, lam, t) for robot in ("lwr", "powercube6", "lwr_dual14") for lam in (0.1, 1e-3) for t in hp.TOOLS]


def _numpy_rows(chain, params, w, tool16):
    from oracle import vfik_numpy as vn
    from vfclik_amd import _abi
    pd = _abi.params_to_dict(params)
    out = {k: np.zeros((hp.B_ARMS, m)) for k, m in (("qdot_vf", chain.n), ("pose", 16), ("pose_nt", 16), ("v6", 6))}
    tools = np.broadcast_to(tool16, (hp.B_ARMS, 16))
    for b in NP_ARMS:
        fd = {int(f["id"]): [float(f["force"]), int(f["type"]), f["p"][:_abi.FIELD_NPARAMS[int(f["type"])]].tolist()]
              for f in w["fields"][b][:w["nfields"][b]]}
        arm = vn.ArmCycle(chain.B, chain.jtype, chain.q_lo, chain.q_hi, pd)
        arm.set_fields(fd)
        got = arm.cycle(w["q"][b].tolist(), tool=tools[b].tolist())
        for k in out:
            out[k][b] = got[k]
    return out


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-lam%g-%s" % c)
def test_oracles_against_the_reference(oracle_c, case, io_dtype):
    robot, lam, tname = case
    chain, params, w, kinds, eps, orc, ref, R, tl = hp.oracle_tool_case(oracle_c, robot, io_dtype, lam, tname)
    assert params.flags == 0 and np.all(orc["status"] == 0)
    rat, err = hp.ratio(orc["qdot_vf"], ref)
    perr = max(hp.error(orc["pose"], ref, "pose").max(), hp.error(orc["pose_nt"], ref, "pose_nt").max())
    b = int(np.argmax(rat))
    shift = ref["qshift"] / np.abs(ref["qdot"]).max(axis=1)
    print("%-11s %s lambda %-6g %-8s C oracle R %.3f (arm %d kind %d eps %g, err %.2e, cond %.2e), pose err %.2e, max shift / qdot %.2f, residual %.1e"
          % (robot, np.dtype(io_dtype).name, lam, tname, R, b, kinds[b], eps[b], err[b], ref["cond"][b], perr, shift.max(), ref["resid"].max()))
    assert ref["resid"].max() < hp.RESIDUAL_BAR
    assert np.all(np.isfinite(orc["qdot_vf"])) and np.abs(ref["qdot"]).max() > 0.1
    # the tool is really on: the tip is off the flange (per-arm: the seeded offsets can bring it nearer), and the point shift moves qdot
    lever = np.linalg.norm(ref["pose"][:, [3, 7, 11]] - ref["pose_nt"][:, [3, 7, 11]], axis=1)
    assert lever.min() > (0.05 if tname == "per-arm" else 0.15) and ref["qshift"].max() > 1e-2
    assert perr < POSE_BAR
    assert np.all(rat <= K_ORACLE), (R, b, kinds[b], eps[b])
    # the NumPy restatement, on its own twists
    npo = _numpy_rows(chain, params, w, tl[2])
    arms = list(NP_ARMS)
    assert np.abs(npo["v6"][arms] - orc["v6"][arms]).max() < 1e-9
    wy, wq = hp.weights("unit", chain.n)
    refn = hp.reference((robot, np.dtype(io_dtype).name, "mixed"), chain, w["q"], npo["v6"], lam, wy, wq, "unit", tool=tl[2], tname=tname, arms=arms)
    ratn = hp.ratio(npo["qdot_vf"][arms], {k: v[arms] for k, v in refn.items()})[0]
    perrn = max(hp.error(npo["pose"], refn, "pose")[arms].max(), hp.error(npo["pose_nt"], refn, "pose_nt")[arms].max())
    print("%-11s %s lambda %-6g %-8s NumPy    R %.3f, pose err %.2e" % (robot, np.dtype(io_dtype).name, lam, tname, ratn.max(), perrn))
    assert perrn < POSE_BAR and np.all(ratn <= K_ORACLE), (ratn.max(), perrn)


@pytest.mark.parametrize("io_dtype", IO, ids=["f32", "f64"])
def test_every_tool_has_the_defect_its_kind_names(io_dtype):
    """max |Rtool Rtool^T - I| per tool, in the band of its kind: below 1e-15 (a rotation to the last bit), 1e-8 .. 1e-7 (rounded to
    float32), 1e-5 .. 1e-3 (typed with 3 or 4 decimals) -- no later edit makes every tool orthonormal again."""
    for name in hp.TOOLS:
        sent, per_arm, seen = hp.tool(name, io_dtype)
        assert sent.shape == ((hp.B_ARMS, 16) if per_arm else (16,)) and seen.shape == ((hp.B_ARMS, 16) if name == "per-arm" else (16,))
        assert np.array_equal(np.asarray(seen).reshape(-1, 16)[:, 12:], np.tile([0.0, 0.0, 0.0, 1.0], (seen.size // 16, 1)))
        d = hp.defect(seen)
        kinds = hp.per_arm_kinds(io_dtype) if name == "per-arm" else [hp.TOOL_KIND[name]]
        for b, (x, k) in enumerate(zip(d, kinds)):
            lo, hi = hp.DEFECT_BANDS[k]
            assert lo <= x < hi, (name, b, k, x)
        if name == "per-arm":
            assert set(kinds) >= {"exact", "typed"} and (io_dtype == np.float64 or "f32" in kinds)
            assert np.array_equal(seen, seen.astype(io_dtype).astype(np.float64)) and len({tuple(r) for r in seen}) == hp.B_ARMS
        if name == "rows":
            assert np.all(sent == sent[0]) and np.array_equal(seen, sent[0].astype(io_dtype).astype(np.float64))
    # f32 is ONE tool for both I/O types; flat has no inverse
    assert np.array_equal(hp.tool("f32", np.float32)[2], hp.tool("f32", np.float64)[2])
    assert abs(np.linalg.det(hp.tool("flat", io_dtype)[2].reshape(4, 4)[:3, :3])) == 0.0
    # turned is strongly non-symmetric, long's lever is longer than the arm
    Rt = hp.tool("turned", io_dtype)[2].reshape(4, 4)[:3, :3]
    assert np.abs(Rt - Rt.T).max() > 0.5 and np.linalg.norm(hp.tool("long", io_dtype)[2][[3, 7, 11]]) > 1.1


def test_the_reference_without_a_tool_is_what_it_was(golden_dir):
    """tests/golden/hp_reference_notool.npz: the reference of one case (lwr, float64 I/O, lambda 1e-3, the sweep's weights, the mixed poses,
    the C oracle's twists of the day in the record) as the helper returned it before it knew of tools -- every value bit for bit (mpmath;
    the longdouble fall-back is held to what its 64-bit mantissa gives).  The identity tool sent down the tool's path gives the same bits
    again: products with 1 and 0 are exact."""
    g = np.load(os.path.join(golden_dir, "hp_reference_notool.npz"))
    chain, w, kinds, eps = hp.make_case("lwr", np.float64, "mixed")
    wy, wq = hp.weights("weighted", chain.n)
    key = ("lwr", "float64", "mixed")
    ref = hp.reference(key, chain, w["q"], g["v6"], 1e-3, wy, wq, "weighted/record")
    if hp.BACKEND == "mpmath":
        for k in ("qdot", "qdot_lo", "pose", "pose_lo", "cond", "resid"):
            assert np.array_equal(ref[k], g[k]), k
    tol = (ref["cond"] * 2.0 ** -58 * np.abs(ref["qdot"]).max(axis=1))[:, None]
    assert np.all(np.abs((ref["qdot"] - g["qdot"]) + (ref["qdot_lo"] - g["qdot_lo"])) <= tol)
    assert np.abs((ref["pose"] - g["pose"]) + (ref["pose_lo"] - g["pose_lo"])).max() < 2.0 ** -58
    assert np.array_equal(ref["pose_nt"], ref["pose"]) and np.array_equal(ref["pose_nt_lo"], ref["pose_lo"]) and not ref["qshift"].any()
    assert np.array_equal(hp.unit_scale(ref), np.abs(ref["qdot"]).max(axis=1))
    ident = hp.reference(key, chain, w["q"], g["v6"], 1e-3, wy, wq, "weighted/record", tool=np.eye(4).reshape(16), tname="identity")
    for k in ref:
        assert np.array_equal(ident[k], ref[k]), k
