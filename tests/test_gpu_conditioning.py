"""The HIP kernels against the high-precision reference (tests/hp_reference.py) as the IK solve's conditioning worsens: lambda from 0.1
down to 1e-3 (0 on regular poses), arms on and next to the shoulder, elbow and wrist singularities, the zero pose, the nodes and midpoints
of the sin / cos table, and joint angles up to eight turns away -- the cases of tests/test_oracle_conditioning.py, which holds the C oracle
to the same reference on the CPU and documents the poses' construction.

Only quantities that are continuous in the inputs are held: qdot_vf (= qdot_out without a module flag) and the pose.  No arm sits on a
decision threshold, and with the nullspace module on (family f) its rank decisions, hence qdot_null, qdot_out and status, are not compared.

Bar per arm b and component i:

    |got - reference| <= max(S, K cond_b u max_i |qdot_b,i|)  [+ 2^-24 |qdot_b,i| at float32 I/O: half an ulp of the store]

  S     the suite's bar, 1e-9 at float64 I/O and 1e-6 at float32: nothing that passes at the default lambda is held tighter here;
  u     2^-53; cond_b = (s1^2 + lambda^2) / (s6^2 + lambda^2) of the arm's weighted Jacobian;
  K     8 max(1, R), R the C oracle's worst ratio err / (cond u |qdot|) on the same case, computed here from the reference, never from the
        kernel.  The 8 over a plain-double solve: the kernel sums in another order with fused multiply-adds; its sin / cos are good to
        about 2 ulp against libm's half, and a perturbation delta of J moves the solution by about cond delta; the table-driven sin / cos
        adds a rounded table entry -- together a factor of 4-5.  It does not let through a pivot reciprocal that is 30-90 u off, which
        is what a single Newton step on the hardware's reciprocal estimate leaves.

Kernel families, each asserted from Engine.launched_kernels (a change of the launch plan cannot silently move a case onto another kernel):

  a  lean, one lane per arm          qdot_out and status alone, no eight-lanes kernel
  b  published rows                  qdot_out, qdot_vf, pose, status
  c  eight lanes per arm             chains of up to 8 joints, small-batch cap 4096
  d  shared weights                  a and c with the sweep's weights in the batch's params (the WTSC variants where they are built:
                                     eight lanes, and float32 I/O of chains of up to 7 joints; the general variants elsewhere)
  e  per-arm weights                 every row the sweep's weights but one arm's wq[1] (its reference uses its own row): general variants
  f  nullspace module                NULLSPACE | MIXER: the solve shared with the projector (chains of 8 joints and more: G from A)

The measured ratios are printed per case and family; with VFIK_CONDITIONING_TABLE=<file> the table is also written there (the record kept
in profiles/conditioning_accuracy.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_reference as hp  # noqa: E402
import kernel_variants as kv  # noqa: E402

ARM_E, WQ1_E = 37, 0.8     # family e: this arm's wq[1] (kind 1, eps 1e-6 on the mixed poses)
_TABLE = []


def _names(eng):
    names = eng.launched_kernels()
    assert names, "no kernel recorded"
    return [kv.parse(n) for n in names]


def _assert_family(vs, fam, nj, io_dtype, wname):
    t = "float" if io_dtype == np.float32 else "double"
    for v in vs:
        a = v.args
        assert a["NJ"] == nj and a["T"] == t, v.name
        wtsc = bool(a["D"] & 4)
        if fam in ("c", "dc"):
            assert v.kernel == "cycle_sub8_kernel_x" and wtsc == (fam == "dc"), v.name
        elif fam == "a":
            assert v.kernel == "cycle_kernel_s" and a["LEAN"] == 1 and a["PL"] and a["FASTF"] and not a["NS"] and not wtsc, v.name
        elif fam == "b":
            assert v.kernel == "cycle_kernel_x" and a["LEAN"] == 3 and a["PL"] and a["FASTF"] and not a["NS"] and not wtsc, v.name
        elif fam == "da":   # the lean launch with shared weights: WTSC where it is built, the general variants elsewhere
            if io_dtype == np.float32 and nj <= 7:
                assert v.kernel == "cycle_kernel_s" and a["LEAN"] == 1 and a["PL"] and wtsc, v.name
            else:
                assert v.kernel == "cycle_kernel_x" and not a["PL"] and a["LEAN"] == 0 and not wtsc, v.name
        elif fam == "e":
            assert v.kernel == "cycle_kernel_x" and not a["PL"] and a["LEAN"] == 0 and not a["NS"], v.name
        elif fam == "f":
            assert v.kernel == "cycle_kernel_x" and a["NS"] and a["PL"] and a["FASTF"] and a["LEAN"] == 3, v.name
        else:
            raise AssertionError(fam)


def _engine_env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c as oc
    from vfclik_amd import _abi, engine
    oc.build()
    return oc, engine, _abi


def _run(engine, chain, w, params, io_dtype, small, want, arm_weights=None):
    eng = engine.Engine(chain, hp.B_ARMS, io_dtype=io_dtype, max_slots=4, params=params)
    try:
        eng.set_small_batch_kernel(small)
        eng.set_fields(w["fields"], w["nfields"])
        if arm_weights is not None:
            eng.set_arm_weights(wy=arm_weights[0], wq=arm_weights[1])
        assert eng.field_path == 1
        eng.launched_kernels()    # (clears the record)
        got = eng.step_host(w["q"], want=want)
        assert eng.small_batch_launches == (1 if small else 0)
        return got, _names(eng)
    finally:
        eng.close()


def _write_table():
    path = os.environ.get("VFIK_CONDITIONING_TABLE")
    if not path:
        return
    with open(path, "w") as f:
        f.write("# worst err / (cond u max|qdot|) per case, C oracle and each kernel family, against the 50-digit reference\n")
        f.write("# (float32: half an ulp of the stored value taken off the error first); `bar`: worst err / bar of the case\n")
        f.write("%-11s %-7s %-7s %-8s %9s  %s\n" % ("robot", "io", "lambda", "weights", "oracle", "family: ratio (kind, eps of the worst arm)"))
        for head, R, rows in _TABLE:
            f.write("%-11s %-7s %-7g %-8s %9.3f  " % (head + (R,)))
            f.write("  ".join("%s: %.3f (%d, %g)" % (what, r, k, e) for what, r, k, e, _ in rows))
            f.write("  bar: %.3f\n" % max(o for *_, o in rows))


@pytest.mark.gpu
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", hp.cases(), ids=hp.case_id)
def test_kernels_against_the_reference(case, io_dtype):
    robot, lam, wname, poses = case
    oc, engine, abi = _engine_env()
    chain, params, w, kinds, eps, orc, ref, R = hp.oracle_case(oc, robot, io_dtype, lam, wname, poses)
    nj, S = chain.n, hp.S_BAR[io_dtype]
    assert np.all(orc["status"] == 0)
    print("\n%s %s lambda %g %s: oracle ratio %.3f, max cond %.3e" % (robot, np.dtype(io_dtype).name, lam, wname, R, ref["cond"].max()))
    failures, row = [], []
    lean, rows = ("qdot_out", "status"), ("qdot_out", "qdot_vf", "pose", "status")
    runs = [("a" if wname == "unit" else "da", 0, lean)]
    if wname == "unit":
        runs.append(("b", 0, rows))
    if nj <= 8:
        runs.append(("c" if wname == "unit" else "dc", 4096, lean))
    for fam, small, want in runs:
        got, vs = _run(engine, chain, w, params, io_dtype, small, want)
        _assert_family(vs, fam, nj, io_dtype, wname)
        if not np.array_equal(got["status"], orc["status"]):
            failures.append("%s: status differs on %d arms" % (fam, int((got["status"] != orc["status"]).sum())))
        for k in want[:-1]:
            if k == "pose":
                perr = hp.error(got[k], ref, "pose").max()
                print("    %-28s max err %.3e" % (fam + " pose", perr))
                if not (np.all(np.isfinite(got[k])) and perr <= S):
                    failures.append("%s: pose err %.3e" % (fam, perr))
            else:
                hp.check_qdot(got[k], ref, io_dtype, R, "%s %s" % (fam, k), kinds, eps, failures, row if k == want[0] else None)
    if wname == "weighted":   # e: per-arm weights, one arm's wq[1] its own
        wy, wq = hp.weights(wname, nj)
        wya, wqa = np.tile(wy, (hp.B_ARMS, 1)), np.tile(wq, (hp.B_ARMS, 1))
        wqa[ARM_E, 1] = WQ1_E
        p1 = abi.default_params(wy=wy, wq=list(wqa[ARM_E]) + [1.0] * (abi.MAX_JOINTS - nj), **{"lambda": lam})
        one = slice(ARM_E, ARM_E + 1)
        o1 = oc.cycle_batch(chain, p1, w["q"][one], w["fields"][one], w["nfields"][one], want=("qdot_vf", "v6", "status"))
        assert np.array_equal(o1["v6"], orc["v6"][one]) and o1["status"][0] == 0
        ref_e = hp.reference((robot, np.dtype(io_dtype).name, poses), chain, w["q"], orc["v6"], lam, wya, wqa, "arm%d" % ARM_E)
        if nj > 6 or lam >= 1e-2:   # the weight acts (a square Jacobian's undamped solve J^-1 tw does not depend on the weights)
            assert np.abs(ref_e["qdot"][ARM_E] - ref["qdot"][ARM_E]).max() > 1e-3 * np.abs(ref["qdot"][ARM_E]).max()
        oq = orc["qdot_vf"].copy()
        oq[ARM_E] = o1["qdot_vf"][0]
        R_e = float(hp.ratio(oq, ref_e)[0].max())
        got, vs = _run(engine, chain, w, abi.default_params(**{"lambda": lam}), io_dtype, 0, lean, arm_weights=(wya, wqa))
        _assert_family(vs, "e", nj, io_dtype, wname)
        if not np.all(got["status"] == 0):
            failures.append("e: status")
        hp.check_qdot(got["qdot_out"], ref_e, io_dtype, R_e, "e qdot_out", kinds, eps, failures, row)
    else:                     # f: the nullspace module; qdot_vf alone is compared
        pf = abi.Params.from_buffer_copy(params)
        pf.flags = abi.F_NULLSPACE | abi.F_MIXER
        got, vs = _run(engine, chain, w, pf, io_dtype, 0, ("qdot_out", "qdot_vf", "status"))
        _assert_family(vs, "f", nj, io_dtype, wname)
        hp.check_qdot(got["qdot_vf"], ref, io_dtype, R, "f qdot_vf", kinds, eps, failures, row)
    _TABLE.append(((robot, np.dtype(io_dtype).name, lam, wname), R, row))
    _write_table()
    assert not failures, "%d failures:\n" % len(failures) + "\n".join(failures)
