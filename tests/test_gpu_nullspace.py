"""The HIP kernels' nullspace module against the high-precision reference (tests/hp_nullspace.py) as J loses rank: restrict / nullspace /
move_in_nullspace, the joint-limit task, check_limits and the mixer behind them, on the cases of tests/test_oracle_nullspace.py (which
holds the C oracle to the same reference on the CPU and documents the poses, the zone, the ambiguous sets and their caps).

The module has four implementations, each losing accuracy with sigma_1 / sigma_6 in its own way: nullspace_core's one pass of modified
Gram-Schmidt (chains of up to 7 joints), the null vector's cold and warm paths, and for chains of 8 and more joints the joint-limit task's
projector through the LDL^T of J J^T in three code forms (accumulated with the Jacobian, GLATE, GLATE + ZLATE).  The last follows the
stated rule of VFIK_PROJ_ROW_MIN (include/vfik_types.h): before it did, the lwr_dual14 arms 1e-9 and 1e-6 rad from the zero pose
(sigma_6 / sigma_1 from 1.2e-10 to 3e-7) got a projected task that was off by 0.2 to 1.2 max|z| from the oracle's.

Bar per arm outside the zone and component (hp_nullspace.bar): max(S, K u (sigma_1 / sigma_6) scale) null_gain, K = 8 max(1, R), R the C
oracle's worst ratio on the same case (never the kernel's), half an ulp of the stored value added at float32 I/O; scale = 1 for v, max|z|
for Pz, |c0| + max|z| for both.  A lean launch publishes qdot_out alone: its bar is |w0| (hp_reference.bars of qdot_vf, the reference's
solve fed the oracle's twist) + |w1| (the bar above), with the mixer on and weights (1, 0.7).

Parameter sets (hp_nullspace.PSETS), each over the mixed poses: `v` c0 = +-1 per arm without the joint-limit task; `Pz` c0 = 0 with it;
`both` at the default lookahead (the stop decision).  Chains: lwr, powercube6 (no nullspace: Pz = 0 within the bar) and lwr_dual14 (/control
is handed over and must be ignored).

Kernel families, each asserted from Engine.launched_kernels:
  pub     published rows (qdot_null, qdot_out, qdot_vf, status)        cycle_kernel_x, LEAN 3, plain, straight-line field path
  lean    qdot_out alone, no /control (set `Pz`: a launch with /control is not lean)   cycle_kernel_s, LEAN 1
  sub8    the eight-lanes kernel with the module (lwr only: it serves chains of up to 7 joints)
  and for lwr_dual14 the three forms of the long chains' projector, set `Pz`:
  acc     plain, straight-line field path, both I/O types: accumulated with the Jacobian (pub and lean above)
  wts     IK weights in the batch's params: GLATE at float32, GLATE + ZLATE at float64 (the general variants; qdot_null, status)
  frac    plain, general field path (one fractional decay order), float32, lean: GLATE (qdot_out)
  lim     set `both` with narrow per-arm limits (hp_nullspace.narrow_limits): the general variants, LEAN 0; arms really stop
  roll    the start of sequence A as one rollout of 2 cycles (the stored vector as doubles in registers): q afterwards

Measured (MI355X; per case and family in profiles/nullspace_accuracy.txt, written by this file with VFIK_NULLSPACE_TABLE=<file>): the
oracle's R is 0.22-0.46 on powercube6 and lwr and 1.2-1.3 on lwr_dual14; the kernels' worst ratio err / (u sigma_1 / sigma_6 scale
null_gain) of qdot_null is 0.90 on powercube6, 0.83 (one lane per arm) and 0.87 (eight lanes) on lwr -- the arm at sigma_6 / sigma_1 =
4.3e-8 is at 0.83 --, 7.7 on lwr_dual14 (against K = 9.8; the absolute error there is 2e-15, far under S); sequence A stays below 0.48
at every step on both mappings; a lean launch's qdot_out is at 0.07 of its bar at float32 I/O.

What a wrong kernel does here, measured once with scratch builds (each run of this file, nothing repeated):
  * the long chains' pivot rule put back to 1e-12: the lwr_dual14 sets `Pz` and `both` fail at both I/O types, on the kind-3 arms at eps
    1e-6 and 1e-3 (errors of 2e-8 to 6e-5), and nothing else fails.  This is the stated-rule form of the defect: under the rule the
    reference itself drops the rows of the arms at eps 0 and 1e-9 (their pivots are below BOTH thresholds, so those arms cannot tell the
    old guard from the new one and are held only to what both compute), and it is at eps 1e-6 and 1e-3 that 1e-12 keeps rows which the
    normal equations cannot resolve.  Five of the eps 1e-3 arms have a pivot within a factor of 4 of the rule and are zone.
  * nullspace_core's rank test at 1e-12 instead of 1e-24: arm 7 of lwr (hp_nullspace.ELBOW_ARM: sigma_6 / sigma_1 = 3.8e-10, squared row
    residual 3e-14 of the squared length) reports VFIK_ST_NULL_AMBIGUOUS in every lwr case and in sequence A;
  * the cold path without its second projection: |J v| / sigma_1 of the published vector (hp_nullspace.check_residual, float64 I/O)
    is over its bar of 32 u on 29 arms of set `v` and of the sequence's cold steps, by up to 1.5e8 u; the bar of qdot_null itself,
    8 u sigma_1 / sigma_6, cannot see it;
  * the warm path's 1e-2 set to 1: the same residual is over 27 u on 25 arms at the sequence's two-projection step, by up to 7 500 u.
The unmutated kernels' residual is at most 3.3 u, the oracle's 4.8 u.

The stop decision is taken both ways: on lwr, regular arms sit 0.02 rad from a limit of the chain and 8 of them stop (sets `v` and `both`,
one lane and eight lanes per arm); under narrow per-arm limits (family lim, the general variants) 14 arms of lwr and 21 of lwr_dual14
stop and as many with limits of the same kind do not; powercube6 has no nullspace and never stops.  Asserted on the reference."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_nullspace as hn  # noqa: E402
import hp_reference as hp  # noqa: E402
import kernel_variants as kv  # noqa: E402

PUB = ("qdot_null", "qdot_out", "qdot_vf", "status")
LEAN = ("qdot_out",)
_TABLE = []


def _engine_env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c as oc
    from vfclik_amd import _abi, engine
    oc.build()
    return oc, engine, _abi


def _run(engine, case, params, io_dtype, small, want, fields=None, control=True, limits=False):
    chain, w = case["chain"], case["w"]
    eng = engine.Engine(chain, hp.B_ARMS, io_dtype=io_dtype, max_slots=4, params=params)
    try:
        eng.set_small_batch_kernel(small)
        eng.set_fields(w["fields"] if fields is None else fields, w["nfields"])
        path = eng.field_path
        eng.launched_kernels()    # (clears the record)
        got = eng.step_host(w["q"], null_control=case["ctrl"] if control else None, want=want,
                            q_lo=case["q_lo"] if limits else None, q_hi=case["q_hi"] if limits else None)
        assert eng.small_batch_launches == (1 if small else 0)
        names = eng.launched_kernels()
        return got, [kv.parse(x) for x in names], path
    finally:
        eng.close()


def _assert_family(vs, fam, nj, io_dtype):
    t = "float" if io_dtype == np.float32 else "double"
    assert vs, "no kernel recorded"
    for v in vs:
        a = v.args
        assert a["NJ"] == nj and a["T"] == t and a["NS"], v.name
        if fam == "pub":
            assert v.kernel == "cycle_kernel_x" and a["LEAN"] == 3 and a["PL"] and a["FASTF"], v.name
        elif fam == "lean":
            assert v.kernel == "cycle_kernel_s" and a["LEAN"] == 1 and a["PL"] and a["FASTF"], v.name
        elif fam == "sub8":
            assert v.kernel in ("cycle_sub8_kernel", "cycle_sub8_kernel_x"), v.name
        # cycle_body's predicates, as this file read them (a change there must be followed here):
        #   GLATE = FUSEP && (!PLAIN || (!FASTF && sizeof(T) == 4 && !(LEAN == 0 && NJ >= 12)));   ZLATE = GLATE && sizeof(T) == 8
        elif fam == "wts":     # IK weights: the general variants, !PLAIN -> GLATE (and ZLATE at float64 I/O)
            assert v.kernel == "cycle_kernel_x" and not a["PL"] and a["LEAN"] == 0, v.name
        elif fam == "frac":    # plain, general field path, float32, LEAN 1 (LEAN 0 of 12+ joints is excepted) -> GLATE
            assert v.kernel == "cycle_kernel_x" and a["PL"] and not a["FASTF"] and a["LEAN"] == 1 and t == "float" and nj >= 8, v.name
        elif fam == "lim":     # per-arm limits: the general variants
            assert v.kernel == "cycle_kernel_x" and a["LEAN"] == 0 and not a["ROLL"], v.name
        elif fam == "roll":
            assert v.kernel in ("cycle_kernel_x", "cycle_kernel_s") and a["ROLL"], v.name
        else:
            raise AssertionError(fam)


def _vf_reference(oc, case, robot, io_dtype, v6, qdot_vf, wkey="unit"):
    """hp_reference's solve fed the oracle's twist, its bar and the oracle's ratio on it"""
    chain, params, w = case["chain"], case["params"], case["w"]
    wy, wq = hp.weights("unit", chain.n)
    ref = hp.reference((robot, np.dtype(io_dtype).name, hn.POSES), chain, w["q"], v6, params.lambda_, wy, wq, wkey)
    R = float(hp.ratio(qdot_vf, ref)[0].max())
    return ref, hp.bars(ref, io_dtype, R)


def _write_table():
    path = os.environ.get("VFIK_NULLSPACE_TABLE")
    if not path:
        return
    with open(path, "w") as f:
        f.write("# worst err / (u sigma_1 / sigma_6 scale null_gain) of qdot_null per case, C oracle (R) and each kernel family, against the 50-digit\n")
        f.write("# reference (float32: half an ulp of the stored value taken off first); `/bar` entries: worst err / bar of a lean launch's qdot_out\n")
        f.write("%-11s %-7s %-5s %8s  %-28s %s\n" % ("robot", "io", "set", "oracle R", "zone / sign-amb / stop-amb", "family: ratio (kind, eps of the worst arm)"))
        for head, R, counts, rows in _TABLE:
            f.write("%-11s %-7s %-5s %8.3f  %-28s " % (head + (R, "%d / %d / %d of %d" % counts)))
            f.write("  ".join("%s: %.3f (%d, %g)" % r for r in rows) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("pset", hn.PSETS)
@pytest.mark.parametrize("robot", hn.NS_ROBOTS)
def test_kernels_against_the_reference(robot, pset, io_dtype):
    oc, engine, abi = _engine_env()
    case = hn.oracle_case(oc, robot, io_dtype, pset)
    chain, params, ref, cyc, kinds, eps, orc = (case[k] for k in ("chain", "params", "ref", "cyc", "kinds", "eps", "orc"))
    nj, g = chain.n, params.null_gain
    hn.assert_caps(ref, cyc, kinds, "%s %s" % (robot, pset))      # on the reference, before any GPU number
    K = hp.K_MARGIN * max(1.0, case["R"])
    scale, expect = case["scale"], hn.expected_status(nj)
    allowed = hn.ST_LIMIT_STOP | hn.ST_NULL_AMBIGUOUS
    print("\n%s %s %s: oracle R %.3f, K %.1f" % (robot, np.dtype(io_dtype).name, pset, case["R"], K))
    failures, row = [], []
    refvf, vf_bar = _vf_reference(oc, case, robot, io_dtype, orc["v6"], orc["qdot_vf"])
    null_bar = hn.bar(ref, io_dtype, K, scale) * abs(g)
    # (a lean launch takes no /control: it exists in the set without c0 alone)
    R_res = 0.0
    if pset == "v" and nj == 7:
        R_res = hn.check_residual(orc["qdot_null"], orc["status"], case["ctrl"][:, 0], g, (robot, np.dtype(io_dtype).name, hn.POSES), chain,
                                  case["w"]["q"], ref, cyc, np.float64, np.inf, "oracle", kinds, eps, failures)
    if pset != "Pz" and nj == 7:
        hn.assert_stops(ref, cyc, "%s %s" % (robot, pset), 4)     # the stop decision is there to be taken, both ways
    runs = [("pub", 0, PUB)] + ([("lean", 0, LEAN)] if pset == "Pz" else []) + ([("sub8", 4096, PUB)] if robot == "lwr" else [])
    for fam, small, want in runs:
        got, vs, path = _run(engine, case, params, io_dtype, small, want, control=fam != "lean")
        assert path == 1
        _assert_family(vs, fam, nj, io_dtype)
        if "qdot_null" in want:
            hn.check_zone(got["qdot_null"], got["status"], ref, case["ctrl"][:, 0], case["jl"], g, allowed, fam, failures,
                          others=(got["qdot_out"], got["qdot_vf"]))
            hn.check_null(got["qdot_null"], got["status"], ref, cyc, io_dtype, K, scale, g, expect, fam + " qdot_null", kinds, eps, failures, row)
            hp.check_qdot(got["qdot_vf"], refvf, io_dtype, float(hp.ratio(orc["qdot_vf"], refvf)[0].max()), fam + " qdot_vf", kinds, eps, failures)
            if pset == "v" and nj == 7:   # the published vector's own residual (hp_nullspace.check_residual), K from the oracle's
                hn.check_residual(got["qdot_null"], got["status"], case["ctrl"][:, 0], g, (robot, np.dtype(io_dtype).name, hn.POSES), chain,
                                  case["w"]["q"], ref, cyc, io_dtype, hp.K_MARGIN * max(1.0, R_res), fam, kinds, eps, failures, row)
        hn.check_out(got["qdot_out"], ref, cyc, refvf, vf_bar, null_bar, hn.MIX_W, g, io_dtype, fam + " qdot_out", kinds, eps, failures,
                     row if fam == "lean" else None)
    if robot == "lwr_dual14" and pset == "Pz":
        # wts: the sweep's IK weights in the batch's params (the projector does not depend on them: the same reference and R)
        wy, wq = hp.weights("weighted", nj)
        pw = hn.pset_params(pset, wy=wy, wq=list(wq) + [1.0] * (abi.MAX_JOINTS - nj))
        got, vs, path = _run(engine, case, pw, io_dtype, 0, ("qdot_null", "status"))
        _assert_family(vs, "wts", nj, io_dtype)
        hn.check_zone(got["qdot_null"], got["status"], ref, 0.0, True, g, allowed, "wts", failures)
        hn.check_null(got["qdot_null"], got["status"], ref, cyc, io_dtype, K, scale, g, expect, "wts qdot_null", kinds, eps, failures, row)
        if io_dtype == np.float32:
            # frac: one fractional decay order puts the batch on the general field path; the twist is the oracle's for THOSE fields
            fields = case["w"]["fields"].copy()
            fields["p"][0, 1, 5] = 2.5
            of = oc.cycle_batch(chain, params, case["w"]["q"], fields, case["w"]["nfields"], null_control=0.0 * case["ctrl"],
                                want=("qdot_vf", "v6", "status"))
            rf, rf_bar = _vf_reference(oc, case, robot, io_dtype, of["v6"], of["qdot_vf"], wkey="unit-frac")
            got, vs, path = _run(engine, case, params, io_dtype, 0, LEAN, fields=fields, control=False)
            assert path != 1
            _assert_family(vs, "frac", nj, io_dtype)
            hn.check_out(got["qdot_out"], ref, cyc, rf, rf_bar, null_bar, hn.MIX_W, g, io_dtype, "frac qdot_out", kinds, eps, failures, row)
    if pset == "both":
        # lim: narrow per-arm limits (hp_nullspace.narrow_limits), under which arms of the chains with a nullspace really stop
        lc = hn.limits_case(oc, robot, io_dtype)
        if nj > 6:
            hn.assert_stops(lc["ref"], lc["cyc"], robot + " lim", 8)
        Kl = hp.K_MARGIN * max(1.0, lc["R"])
        got, vs, path = _run(engine, lc, params, io_dtype, 0, PUB, limits=True)
        _assert_family(vs, "lim", nj, io_dtype)
        hn.check_zone(got["qdot_null"], got["status"], lc["ref"], lc["ctrl"][:, 0], True, g, allowed, "lim", failures)
        hn.check_null(got["qdot_null"], got["status"], lc["ref"], lc["cyc"], io_dtype, Kl, lc["scale"], g, expect, "lim qdot_null", kinds, eps, failures, row)
        hn.check_out(got["qdot_out"], lc["ref"], lc["cyc"], refvf, vf_bar, hn.bar(lc["ref"], io_dtype, Kl, lc["scale"]) * abs(g), hn.MIX_W, g,
                     io_dtype, "lim qdot_out", kinds, eps, failures)
    held = ~ref["zone"]
    _TABLE.append(((robot, np.dtype(io_dtype).name, pset), case["R"],
                   (int((~held).sum()), int((cyc["sign_amb"] & held).sum()), int((cyc["stop_amb"] & held).sum()), len(held)), row))
    _write_table()
    assert not failures, "%d failures:\n" % len(failures) + "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_cycle_sequence_a_through_separate_launches(io_dtype):
    """hp_nullspace.sequence_a on the 7-joint chain, one launch per step, so that the stored vector makes its round trip through the float32
    state: cold start, warm with one projection, warm with two, cold again after a jump -- lanes built for each branch beside others in
    every wave and group of eight (tests/test_oracle_nullspace.py asserts that on the CPU).  Set `v`: qdot_null = null_gain c0 v holds the
    vector each path produces, sign continuity included.  One lane per arm and eight lanes per arm."""
    oc, engine, abi = _engine_env()
    seq = hn.sequence_a(io_dtype)
    chain, w, params, kinds, eps = (seq[k] for k in ("chain", "w", "params", "kinds", "eps"))
    outs, Rs = hn.sequence_oracle(oc, seq)
    failures, row = [], []
    Rres = [hn.check_residual(outs[k]["qdot_null"], outs[k]["status"], seq["ctrl"][:, 0], params.null_gain, seq["keys"][k], chain, seq["qs"][k],
                              seq["refs"][k], seq["cycs"][k], np.float64, np.inf, "oracle " + hn.SEQ_STEPS[k], kinds, eps, failures) for k in range(4)]
    for fam, small in (("pub", 0), ("sub8", 4096)):
        eng = engine.Engine(chain, hp.B_ARMS, io_dtype=io_dtype, max_slots=4, params=params)
        try:
            eng.set_small_batch_kernel(small)
            eng.set_fields(w["fields"], w["nfields"])
            eng.launched_kernels()
            for k in range(4):
                got = eng.step_host(seq["qs"][k], null_control=seq["ctrl"], want=("qdot_null", "qdot_out", "status"))
                ref, cyc = seq["refs"][k], seq["cycs"][k]
                K = hp.K_MARGIN * max(1.0, Rs[k])
                what = "%s %s" % (fam, hn.SEQ_STEPS[k])
                hn.check_zone(got["qdot_null"], got["status"], ref, seq["ctrl"][:, 0], False, params.null_gain,
                              hn.ST_LIMIT_STOP | hn.ST_NULL_AMBIGUOUS, what, failures)
                hn.check_null(got["qdot_null"], got["status"], ref, cyc, io_dtype, K, 1.0, params.null_gain, 0, what, kinds, eps, failures, row)
                hn.check_residual(got["qdot_null"], got["status"], seq["ctrl"][:, 0], params.null_gain, seq["keys"][k], chain, seq["qs"][k], ref,
                                  cyc, io_dtype, hp.K_MARGIN * max(1.0, Rres[k]), what, kinds, eps, failures, row)
            assert eng.small_batch_launches == (4 if small else 0)
            _assert_family([kv.parse(x) for x in eng.launched_kernels()], fam, chain.n, io_dtype)
        finally:
            eng.close()
    _TABLE.append((("lwr", np.dtype(io_dtype).name, "seqA"), max(Rs), (int(seq["refs"][0]["zone"].sum()), int(seq["cycs"][2]["sign_amb"].sum()), 0, hp.B_ARMS), row))
    _write_table()
    assert not failures, "%d failures:\n" % len(failures) + "\n".join(failures)


DT = 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_sequence_a_as_one_rollout_of_two_cycles(io_dtype):
    """The start of sequence A as ONE rollout of 2 cycles with dt = 1e-3: cold, then warm with the stored vector kept as doubles in
    registers.  q afterwards against q + dt (out(q) + out(q + dt out(q))), out = w0 (hp_reference's solve fed the oracle's twist) +
    w1 (this reference's qdot_null, sign continuity included), held as tests/test_gpu_field_edges.py holds its `roll` row: bar dt (bar
    of cycle 1 + bar of cycle 2) + the stored value's half ulp (float32) or 4 u |q| (float64).  Arms in the zone at either cycle, or
    held only up to sign, or stop-ambiguous, must come back finite."""
    oc, engine, abi = _engine_env()
    seq = hn.sequence_a(io_dtype)
    chain, w, params, kinds, eps, ctrl = (seq[k] for k in ("chain", "w", "params", "kinds", "eps", "ctrl"))
    ion, g = np.dtype(io_dtype).name, params.null_gain
    wy, wq = hp.weights("unit", chain.n)
    states = oc.new_states(hp.B_ARMS, chain.n)
    q, prev, sig = seq["qs"][0], None, None
    qbar, held = 0.0, np.ones(hp.B_ARMS, dtype=bool)
    for k, pk in enumerate((hn.POSES, "seq-roll")):
        key = ("lwr", ion, pk)
        o = oc.cycle_batch(chain, params, q, w["fields"], w["nfields"], null_control=ctrl, states=states, want=("qdot_vf", "qdot_null", "v6", "status"))
        ref = hn.reference(key, chain, q, params.jl_gain)
        cyc = hn.cycle(ref, chain.n, ctrl[:, 0], False, g, params.lookahead, io_dtype, q, prev=prev, sig=sig)
        rvf = hp.reference(key, chain, q, o["v6"], params.lambda_, wy, wq, "unit")
        ok = ~ref["zone"] & ~cyc["stop"] & ~cyc["sign_amb"]
        R = float(np.where(ok, hn.error(o["qdot_null"], cyc, "qdot_null").max(axis=1) / (hp.U / np.maximum(ref["gap"], 1e-300) * abs(g)), 0.0).max())
        bar_k = abs(hn.MIX_W[0]) * hp.bars(rvf, io_dtype, float(hp.ratio(o["qdot_vf"], rvf)[0].max())) \
            + abs(hn.MIX_W[1]) * (hn.bar(ref, io_dtype, hp.K_MARGIN * max(1.0, R), 1.0) * abs(g))[:, None]
        qbar = qbar + DT * np.where(np.isfinite(bar_k), bar_k, 0.0)
        held &= ~ref["zone"] & ~cyc["sign_amb"] & ~cyc["stop_amb"]
        out = hn.MIX_W[0] * (rvf["qdot"] + rvf["qdot_lo"]) + hn.MIX_W[1] * (cyc["qdot_null"] + cyc["qdot_null_lo"])
        q = q + DT * out
        prev, sig = cyc["vpub"], cyc["sig"]
    assert held.sum() > hp.B_ARMS // 2
    eng = engine.Engine(chain, hp.B_ARMS, io_dtype=io_dtype, max_slots=4, params=params)
    try:
        eng.set_fields(w["fields"], w["nfields"])
        eng.launched_kernels()
        got = eng.rollout_host(seq["qs"][0], 2, DT, null_control=ctrl, want=("qdot_out", "status"))
        _assert_family([kv.parse(x) for x in eng.launched_kernels()], "roll", chain.n, io_dtype)
    finally:
        eng.close()
    qbar = qbar + (2.0 ** -24 * np.abs(q) if io_dtype == np.float32 else 4 * hp.U * np.abs(q))
    qerr = np.abs(got["q"].astype(np.float64) - q)
    over = np.where(held[:, None], qerr / qbar, 0.0)
    wb = int(np.argmax(over.max(axis=1)))
    print("\nroll %s: %d arms held, worst err / bar %.3f (arm %d kind %d eps %g: err %.3e)" % (ion, held.sum(), over.max(), wb, kinds[wb], eps[wb], qerr[wb].max()))
    assert np.all(np.isfinite(got["q"])) and np.all(np.isfinite(got["qdot_out"]))
    assert over.max() <= 1.0, (wb, kinds[wb], eps[wb], over.max())
