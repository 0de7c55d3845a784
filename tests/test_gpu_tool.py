"""The HIP kernels against the high-precision reference (tests/hp_reference.py) with a hand on the arm: the tool pose (vf:321-332), the
point shift of the twist, Twist.RefPoint(p_ee - p_tip) (vf:456-459), and /pose_no_tool -- with the tools of hp.TOOLS, among them 3 x 3
blocks as a float32 file or a hand-written config holds them (off a rotation by 5e-8 ... 9e-4), equal per-arm rows, per-arm tools and a
block without an inverse.  tests/test_oracle_tool.py holds the C oracle and the NumPy restatement to the same reference on the CPU and
documents the tools; KDL's frame product takes any nine numbers, and so must every kernel: the same tool gives ONE answer, however the
caller sent it.

Bar per arm b and component i (qdot_out, qdot_vf):

    |got - reference| <= max(S, K unit_b)  [+ 2^-24 |qdot_b,i| at float32 I/O: half an ulp of the store]

  S     the suite's bar, 1e-9 at float64 I/O and 1e-6 at float32;  pose and pose_nt are held to S
  unit  cond_b u (max_i |qdot_b,i| + max_i |qdot_shift_b,i|), qdot_shift the reference's solve of the twist (w x AB, 0) alone: w x AB
        can cancel v, and the rounding of either part stays.  Without a tool it is the conditioning sweep's unit.
  K     8 max(1, R), R the C oracle's worst err / unit on the same case -- from the reference and the oracle, never from the kernel
        (tests/test_gpu_conditioning.py accounts for the 8)

The twist stays an input (the oracle's v6): the field at a tool pose whose rotation is no rotation is not this test's.

Kernel families, each asserted from Engine.launched_kernels:

  t-a  lean launch (qdot_out, status)           float32 I/O: cycle_kernel_s, LEAN 1, PL, D & 2 (the shared tool applied by the kernel built
                                                for all-revolute chains); float64 I/O: the general variants, as plan_cycle documents
  t-b  published rows (+ qdot_vf, pose, pose_nt, v6)   float32: the publishing-lean variant with D & 2; float64: general
  t-c  eight lanes per arm (chains the kernel serves, cap 4096)   cycle_sub8_kernel_x with D & 2 at BOTH I/O types; lean, and with pose_nt
  t-f  NULLSPACE | MIXER with the shared tool   only qdot_vf, pose and pose_nt are compared (rank decisions are not this test's)
  t-e  the per-arm tool                         general variants, not PL
  `rows` launches what `typed4` sent with per_arm = 0 launches; `flat` (no inverse) is not a tool of the D & 2 kernels: general variants

Run once against the library of the commit before the block's inverse replaced its transpose (Rtool^T t for the lever arm and
Rt Rtool^T for pose_no_tool in the D & 2 kernels, the latter also in the general variants of chains of 10 joints and more), this file
failed 18 of its 44 cases: typed4, typed3 and rows in t-a / t-b / t-f at float32 I/O and in t-c at both (qdot off by 1e9 ... 2e10 units,
pose_nt by 9.8e-5 / 8.9e-4), f32 in t-c at float64 I/O (pose_nt 6.4e-8), pose_nt of lwr_dual14's per-arm tools and of rand10's typed4
(8.8e-4 / 9.9e-5), and flat at float32 I/O (launched on the D & 2 kernels).  profiles/tool_accuracy.txt keeps both tables.

With VFIK_TOOL_TABLE=<file> the measured ratios are also written there (the record kept in profiles/tool_accuracy.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_reference as hp  # noqa: E402
import kernel_variants as kv  # noqa: E402

LEAN = ("qdot_out", "status")
ROWS = ("qdot_out", "qdot_vf", "pose", "pose_nt", "v6", "status")
LEAN_NT = ("qdot_out", "pose_nt", "status")
_TABLE = []


def _engine_env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c as oc
    from vfclik_amd import _abi, engine
    oc.build()
    return oc, engine, _abi


def _run(engine, chain, w, params, io_dtype, small, want, tl):
    eng = engine.Engine(chain, hp.B_ARMS, io_dtype=io_dtype, max_slots=4, params=params)
    try:
        eng.set_small_batch_kernel(small)
        eng.set_fields(w["fields"], w["nfields"])
        if tl is not None:
            eng.set_tool(tl[0], per_arm=tl[1])
        assert eng.field_path == 1
        eng.launched_kernels()    # (clears the record)
        got = eng.step_host(w["q"], want=want)
        assert eng.small_batch_launches == (1 if small else 0)
        names = eng.launched_kernels()
        assert names, "no kernel recorded"
        return got, [kv.parse(n) for n in names]
    finally:
        eng.close()


def _assert_family(vs, fam, nj, io_dtype):
    t = "float" if io_dtype == np.float32 else "double"
    f32 = io_dtype == np.float32
    for v in vs:
        a = v.args
        assert a["NJ"] == nj and a["T"] == t, v.name
        general = v.kernel == "cycle_kernel_x" and not a["PL"] and a["LEAN"] == 0 and not a["D"]
        if fam == "t-c":
            assert v.kernel == "cycle_sub8_kernel_x" and a["D"] & 2, v.name
        elif fam == "t-a" and f32:
            assert v.kernel == "cycle_kernel_s" and a["LEAN"] == 1 and a["PL"] and a["D"] & 2 and not a["NS"], v.name
        elif fam == "t-b" and f32:
            assert v.kernel == "cycle_kernel_x" and a["LEAN"] == 3 and a["PL"] and a["D"] & 2 and not a["NS"], v.name
        elif fam == "t-f" and f32:
            assert v.kernel == "cycle_kernel_x" and a["LEAN"] == 3 and a["PL"] and a["D"] & 2 and a["NS"], v.name
        elif fam == "t-f":
            assert general and a["NS"], v.name
        elif fam in ("t-a", "t-b", "t-e", "general"):
            assert general and not a["NS"], v.name
        else:
            raise AssertionError(fam)


def _check(got, want, orc, ref, io_dtype, R, fam, kinds, eps, failures, row, status=True):
    S = hp.S_BAR[io_dtype]
    if status and not np.array_equal(got["status"], orc["status"]):
        failures.append("%s: status differs on %d arms" % (fam, int((got["status"] != orc["status"]).sum())))
    first = True
    for k in want:
        if k in ("pose", "pose_nt"):
            perr = hp.error(got[k], ref, k).max()
            print("    %-28s max err %.3e" % (fam + " " + k, perr))
            row.append((fam + " " + k, perr / S, -1, 0.0, perr / S))
            if not (np.all(np.isfinite(got[k])) and perr <= S):
                failures.append("%s: %s err %.3e against %.0e" % (fam, k, perr, S))
        elif k == "v6":
            print("    %-28s max |v6 - oracle| %.3e" % (fam + " v6", np.abs(got[k] - orc["v6"]).max()))
        elif k in ("qdot_out", "qdot_vf"):
            hp.check_qdot(got[k], ref, io_dtype, R, "%s %s" % (fam, k), kinds, eps, failures, row if first else None)
            first = False


def _write_table():
    path = os.environ.get("VFIK_TOOL_TABLE")
    if not path:
        return
    with open(path, "w") as f:
        f.write("# worst err / unit per case, C oracle (R) and each kernel family, against the 50-digit reference; unit = cond u (max|qdot| + max|qdot_shift|)\n")
        f.write("# (float32: half an ulp of the stored value taken off the error first); pose, pose_nt: worst err / S; `bar`: worst err / bar of the case\n")
        f.write("%-11s %-7s %-7s %-8s %7s  %s\n" % ("robot", "io", "lambda", "tool", "oracle", "family output: ratio"))
        for head, R, rows in _TABLE:
            f.write("%-11s %-7s %-7g %-8s %7.3f  " % (head + (R,)))
            f.write("  ".join("%s: %.3g" % (what, r) for what, r, *_ in rows))
            f.write("  bar: %.3g\n" % max(o for *_, o in rows))


def _case(oc, engine, abi, robot, io_dtype, lam, tname, chain=None, poses="mixed"):
    chain, params, w, kinds, eps, orc, ref, R, tl = hp.oracle_tool_case(oc, robot, io_dtype, lam, tname, poses, chain)
    nj = chain.n
    assert np.all(orc["status"] == 0)
    print("\n%s %s lambda %g tool %s: oracle ratio %.3f, max cond %.3e, max shift / qdot %.2f"
          % (robot, np.dtype(io_dtype).name, lam, tname, R, ref["cond"].max(), (ref["qshift"] / np.abs(ref["qdot"]).max(axis=1)).max()))
    failures, row = [], []
    plain_tool = tname is not None and not tl[1] and tname != "flat" and sum(chain.jtype) == 0 or tname == "rows"
    if tname == "per-arm":
        runs = [("t-e", "t-e", 0, ROWS)]
    elif not plain_tool:   # no tool, a chain with a prismatic joint, or a block without an inverse: the general variants
        runs = [("general lean", "general", 0, LEAN), ("general rows", "general", 0, ROWS)]
    else:
        runs = [("t-a", "t-a", 0, LEAN), ("t-b", "t-b", 0, ROWS)]
        if nj <= 8:
            runs += [("t-c", "t-c", 4096, LEAN), ("t-c nt", "t-c", 4096, LEAN_NT)]
    for label, fam, small, want in runs:
        got, vs = _run(engine, chain, w, params, io_dtype, small, want, tl)
        _assert_family(vs, fam, nj, io_dtype)
        if tname == "rows":    # ... and what the same tool launches when it is sent as the shared tool
            vs4 = _run(engine, chain, w, params, io_dtype, small, want, hp.tool("typed4", io_dtype))[1]
            assert [v.name for v in vs] == [v.name for v in vs4], (label, vs, vs4)
        _check(got, want, orc, ref, io_dtype, R, label, kinds, eps, failures, row)
    if plain_tool:
        pf = abi.Params.from_buffer_copy(params)
        pf.flags = abi.F_NULLSPACE | abi.F_MIXER
        want = ("qdot_out", "qdot_vf", "pose", "pose_nt", "status")
        got, vs = _run(engine, chain, w, pf, io_dtype, 0, want, tl)
        _assert_family(vs, "t-f", nj, io_dtype)
        _check(got, want[1:], orc, ref, io_dtype, R, "t-f", kinds, eps, failures, row, status=False)
    _TABLE.append(((robot, np.dtype(io_dtype).name, lam, str(tname)), R, row))
    _write_table()
    assert not failures, "%d failures:\n" % len(failures) + "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", hp.tool_cases(), ids=lambda c: "%s-lam%g-%s" % c)
def test_kernels_against_the_reference_with_a_tool(case, io_dtype):
    robot, lam, tname = case
    oc, engine, abi = _engine_env()
    _case(oc, engine, abi, robot, io_dtype, lam, tname)


def _rand10():
    """the 10-joint chain of tests/test_gpu_parity.py's test_ten_joint_chain_with_prismatic: two prismatic joints, a trailing screw"""
    from vfclik_amd.chain import Chain
    rng = np.random.default_rng(11)
    segs = []
    for i in range(10):
        axis = rng.normal(size=3)
        tip = np.eye(4)
        tip[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        if np.linalg.det(tip[:3, :3]) < 0:
            tip[:3, 0] *= -1
        tip[:3, 3] = rng.uniform(-0.2, 0.2, 3)
        segs.append((1 if i in (2, 7) else 0, axis, tip))
    lo = np.where([s[0] == 1 for s in segs], -0.3, -2.5)
    return Chain.from_segments(segs, lo, -lo, name="rand10")


@pytest.mark.gpu
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("tname", [None, "turned", "typed4"], ids=["identity", "turned", "typed4"])
def test_a_general_chain_with_prismatic_joints(tname, io_dtype):
    """The joint-type blends and the trailing screw of the general variants under the 50-digit reference, on regular poses; with `typed4`
    also the long chains' pose_no_tool, whose rotation the general variants recompose from the tool pose."""
    oc, engine, abi = _engine_env()
    chain = _rand10()
    assert chain.n == 10 and sum(chain.jtype) == 2
    _case(oc, engine, abi, "rand10", io_dtype, 0.1, tname, chain=chain, poses="regular")
