"""The HIP kernels' field evaluation against the 50-digit field reference (tests/hp_field.py) on the edge scenes: every separate
implementation of DESIGN 2.1's field in vfik_kernel.hip -- the uniform-order straight-line path (compact image: orders 0, 1, 2, 5, 20,
127), the uniform repeller image, the three MIXO code paths, the aux block, eval_slot of the general path, the eight-lanes kernel and
probe_kernel -- at the floors, the cap, the gates' kinks, the reduction boundaries of atan2_pos and under cancellation.
tests/test_oracle_field_edges.py holds the C oracle to the same reference on the CPU and asserts that every arm sits where its kind says.

Per cycle scene (LWR, lambda = 0.1; scene 1 at order 5 also on the powercube6):

  pub    the publishing launch: v6 against the reference, qdot_out (= qdot_vf) against hp_reference's solve FED THE REFERENCE TWIST
  lean   the lean launch: qdot_out alone
  sub8   the eight-lanes kernel where the scene admits it (repellers only, one order): qdot_out
  roll   scene 1-o5: one rollout of 2 cycles, q after it against q + dt (qdot_ref(q) + qdot_ref(q + dt qdot_ref(q)))
  probe  Engine.probe_field on the probe scenes, kappa_pose = 0

Bars, per arm (hp_field: E = u (kappa_pose + kappa_rel + (4 + kappa_sum) max|v6|)):

  v6     max(S, K E), K = 8 max(1, R), R the C oracle's worst err / E on the scene (from the reference, never from the kernel)
  qdot   max(S, Ks cond u max|qdot| + K E / (2 lambda)): hp_reference's conditioning term, Ks = 8 max(1, Rs) with Rs the oracle solve's
         ratio on the scene, and the twist's bar through the damped pseudo-inverse, whose norm is at most 1 / (2 lambda)
  float32 I/O adds half an ulp of the stored value; S = 1e-9 / 1e-6 (the suite's).
  Finite-only arms (8 E > 1e-3 max|v6|; none in the scenes as built): every output finite, status 0, |v|, |w| <= speedScale (1 + 1e-12).

Which kernels ran is asserted from Engine.launched_kernels, field_path, mixed_orders and uniform_repellers: compact or uniform image (UNI,
on the publishing launch, whose v6 is compared, as on the lean one), aux block (FUN), general path, the MIXO kernel.  WHICH of the MIXO
kernel's three code paths a wave takes is decided at run time from the wave's order bytes and cannot be read from a kernel name: scenes 3
and 4 give every arm the same two orders slot by slot ((5, 20): a ratio of 4, the 2^j shortcut; (3, 7): no power-of-two ratio, the second
pass), scene 5 three orders and arms with orders of their own (the per-lane path) -- asserted here is only that the MIXO kernel ran on them.

What the sweep can and cannot see of 1 / D.  An error common to the slots of one order multiplies their terms by one factor; normCart
removes it but for the goal's share of the sum.  A library whose compact-image reciprocal square root is scaled by 1 + 1e-13 (90 u) was run
on scenes 1-o5, 1-o20, 1-o127 and 2-o20: it PASSES them -- err / E rises from 1.0 to 10, 20 and 24 on the ratio+-9 arms (magnitude 1, where
the goal's share is largest), an error of 1e-10, under S -- and fails one older test (test_gpu_parity's lean-against-publishing comparison
at 1e-12).  The reciprocal square root's own error is measured directly by tools/ubench_rsqrt.hip, not inferred from this sweep.  The worst err / E per scene
and family is printed; with VFIK_FIELD_TABLE=<file> the table is also written there (the record kept in profiles/field_accuracy.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_field as hf  # noqa: E402
import hp_reference as hp  # noqa: E402
import kernel_variants as kv  # noqa: E402

PUB = ("qdot_out", "qdot_vf", "pose", "v6", "status")
LEAN = ("qdot_out", "status")
DT = 1e-3
# scene -> (field_path, mixed_orders, uniform_repellers)
STRUCTURE = {"3": (1, True, False), "4": (1, True, False), "5": (1, True, True), "6": (2, False, False), "7": (0, False, False)}
_TABLE = {}


def _structure(sid):
    if sid.startswith("1-"):
        return (1, False, False)
    if sid.startswith("2-"):
        return (1, False, True)
    return STRUCTURE[sid]


def _env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c as oc
    from vfclik_amd import engine
    oc.build()
    return oc, engine


def _assert_kernels(names, sid, fam, nj, io_dtype, failures):
    """every kernel of the launch is the code path the scene was built for"""
    path, mixed, uni = _structure(sid)
    t = "float" if io_dtype == np.float32 else "double"
    if not names:
        failures.append("%s: no kernel recorded" % fam)
    for name in names:
        v = kv.parse(name)
        a = v.args
        ok = a["NJ"] == nj and a["T"] == t
        if fam == "sub8":
            ok = ok and v.kernel == "cycle_sub8_kernel_x"
        elif mixed:     # the MIXO variants are instantiated through cycle_kernel_m
            ok = ok and v.kernel == "cycle_kernel_m" and a["LEAN"] == (1 if fam == "lean" else 3) and a["FUN"] == (path == 2)
        else:
            ok = ok and v.kernel in ("cycle_kernel_s", "cycle_kernel_x") and a["FASTF"] == (path > 0) and a["FUN"] == (path == 2)
            if path > 0:
                ok = ok and a["LEAN"] == (1 if fam == "lean" else 3)
                ok = ok and not a.get("MIXO", False)
                ok = ok and a["UNI"] == (uni and path == 1)    # (launches without an aux block read the uniform image)
        if not ok:
            failures.append("%s: launched %s, the scene expects field path %d, mixed %s, uniform %s" % (fam, name, path, mixed, uni))


def _arms(sc, mask):
    return ", ".join("%d %s" % (b, hf.kinds_of(sc, b)) for b in np.flatnonzero(mask)[:40])


def _check_v6(got, ref, io_dtype, R, what, sc, failures, row):
    got = np.asarray(got, dtype=np.float64)
    held = ~ref["finite_only"]
    err = hf.v6_error(got, ref)
    rat = hf.v6_ratio(got, ref, io_dtype)
    over = np.where(held[:, None], err / hf.v6_bar(ref, io_dtype, R), 0.0)
    b, wb = int(np.argmax(rat)), int(np.argmax(over.max(axis=1)))
    print("    %-12s err / E %9.3f (arm %3d %s)  worst err / bar %.3f (arm %d %s: err %.3e, E %.3e)"
          % (what, rat[b], b, hf.kinds_of(sc, b), over.max(), wb, hf.kinds_of(sc, wb), err[wb].max(), ref["E"][wb]))
    row.append((what, rat[b], hf.kinds_of(sc, b), over.max()))
    speed = sc["params"].speed_scale * (1 + 1e-12) + (2.0 ** -24 * sc["params"].speed_scale if io_dtype == np.float32 else 0.0)
    if not np.all(np.isfinite(got)):
        failures.append("%s: %d values are not finite: %s" % (what, int((~np.isfinite(got)).sum()), _arms(sc, ~np.isfinite(got).all(axis=1))))
    elif over.max() > 1.0:
        failures.append("%s: err / bar = %.2f on arm %d (%s): err / E = %.1f against K = %.1f"
                        % (what, over.max(), wb, hf.kinds_of(sc, wb), rat[wb], hp.K_MARGIN * max(1.0, R)))
    elif np.linalg.norm(got[:, :3], axis=1).max() > speed or np.linalg.norm(got[:, 3:], axis=1).max() > speed:
        failures.append("%s: a twist longer than speedScale" % what)


def _qdot_bar(refq, ref, io_dtype, R, Rs):
    K, Ks = hp.K_MARGIN * max(1.0, R), hp.K_MARGIN * max(1.0, Rs)
    arm = np.maximum(hp.S_BAR[io_dtype], Ks * refq["cond"] * hp.U * np.abs(refq["qdot"]).max(axis=1) + K * ref["E"] / (2 * hf.LAMBDA))
    bar = np.repeat(arm[:, None], refq["qdot"].shape[1], axis=1)
    if io_dtype == np.float32:
        bar = bar + 2.0 ** -24 * np.abs(refq["qdot"])
    return bar


def _check_qdot(got, refq, ref, bar, io_dtype, what, sc, failures, row):
    """err against the bar; the printed ratio is err / (Ks-free unit: cond u max|qdot| + E / (2 lambda)), float32's store taken off"""
    got = np.asarray(got, dtype=np.float64)
    held = ~ref["finite_only"]
    err = hp.error(got, refq, "qdot")
    store = 2.0 ** -24 * np.abs(refq["qdot"]) if io_dtype == np.float32 else 0.0
    unit = refq["cond"] * hp.U * np.abs(refq["qdot"]).max(axis=1) + ref["E"] / (2 * hf.LAMBDA)
    rat = np.where(held, np.maximum(err - store, 0.0).max(axis=1) / unit, 0.0)
    over = np.where(held[:, None], err / bar, 0.0)
    b, wb = int(np.argmax(rat)), int(np.argmax(over.max(axis=1)))
    print("    %-12s err / unit %6.3f (arm %3d %s)  worst err / bar %.3f (arm %d %s: err %.3e)"
          % (what, rat[b], b, hf.kinds_of(sc, b), over.max(), wb, hf.kinds_of(sc, wb), err[wb].max()))
    row.append((what, rat[b], hf.kinds_of(sc, b), over.max()))
    if not np.all(np.isfinite(got)):
        failures.append("%s: %d values are not finite: %s" % (what, int((~np.isfinite(got)).sum()), _arms(sc, ~np.isfinite(got).all(axis=1))))
    elif over.max() > 1.0:
        failures.append("%s: err / bar = %.2f on arm %d (%s), err %.3e" % (what, over.max(), wb, hf.kinds_of(sc, wb), err[wb].max()))


def _write_table():
    path = os.environ.get("VFIK_FIELD_TABLE")
    if not path:
        return
    with open(path, "w") as f:
        f.write("# worst err / E per scene and kernel family against the 50-digit field reference (tests/hp_field.py); v6 rows: E = u (kappa_pose +\n"
                "# kappa_rel + (4 + kappa_sum) max|v6|); qdot rows: err / (cond u max|qdot| + E / (2 lambda)); float32: half an ulp of the stored\n"
                "# value taken off the error first; `bar`: worst err / bar of the case; (kinds of the worst arm)\n")
        f.write("%-9s %-7s %7s  %s\n" % ("scene", "io", "oracle", "family: ratio (kinds of the worst arm)"))
        for (sid, io), (R, rows) in _TABLE.items():
            f.write("%-9s %-7s %7.3f  " % (sid, io, R))
            f.write("  ".join("%s: %.3f (%s)" % (what, r, k) for what, r, k, _ in rows))
            f.write("  bar: %.3f\n" % max(o for *_, o in rows))


def _solve_refs(oc, sc, ref, q, key, tag):
    """(reference of the solve fed the reference twist, Rs: the oracle solve's ratio against the reference fed the ORACLE'S twist)"""
    chain = sc["chain"]
    unit = hp.weights("unit", chain.n)
    refq = hp.reference(key, chain, q, ref["v6"], hf.LAMBDA, unit[0], unit[1], (tag, sc["sid"], "ref"))
    orc = oc.cycle_batch(chain, sc["params"], q, sc["w"]["fields"], sc["w"]["nfields"], want=("qdot_vf", "v6", "status"))
    refo = hp.reference(key, chain, q, orc["v6"], hf.LAMBDA, unit[0], unit[1], (tag, sc["sid"], "orc"))
    return refq, float(hp.ratio(orc["qdot_vf"], refo)[0].max())


@pytest.mark.gpu
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("sid", hf.CYCLE_SCENES)
def test_cycle_kernels_against_the_field_reference(sid, io_dtype):
    oc, engine = _env()
    sc, ref, R = hf.oracle_scene(oc, sid, io_dtype)
    chain, w, params = sc["chain"], sc["w"], sc["params"]
    nj = chain.n
    refq, Rs = _solve_refs(oc, sc, ref, w["q"], hf.kin_key(sc), "field")
    bar = _qdot_bar(refq, ref, io_dtype, R, Rs)
    path, mixed, uni = _structure(sid)
    print("\n%s %s: oracle err / E %.3f, oracle solve ratio %.3f, max kappa_sum %.2e, max E %.2e, finite-only arms %d"
          % (sid, np.dtype(io_dtype).name, R, Rs, ref["kappa_sum"].max(), ref["E"].max(), int(ref["finite_only"].sum())))
    failures, row = [], []
    runs = [("pub", 0, PUB), ("lean", 0, LEAN)]
    if path == 1 and not mixed and nj <= 8:
        runs.append(("sub8", 4096, LEAN))
    for fam, small, want in runs:
        eng = engine.Engine(chain, hf.B_ARMS, io_dtype=io_dtype, max_slots=sc["max_slots"], params=params)
        try:
            eng.set_small_batch_kernel(small)
            eng.set_fields(w["fields"], w["nfields"])
            got_structure = (eng.field_path, eng.mixed_orders, eng.uniform_repellers)
            if got_structure != (path, mixed, uni):
                failures.append("%s: (field_path, mixed_orders, uniform_repellers) = %r, expected %r" % (fam, got_structure, (path, mixed, uni)))
            eng.launched_kernels()    # (clears the record)
            got = eng.step_host(w["q"], want=want)
            if eng.small_batch_launches != (1 if small else 0):
                failures.append("%s: %d small-batch launches" % (fam, eng.small_batch_launches))
            names = sorted(eng.launched_kernels())
        finally:
            eng.close()
        print("  %s: %s" % (fam, ", ".join(names)))
        _assert_kernels(names, sid, fam, nj, io_dtype, failures)
        if not np.all(got["status"] == 0):
            failures.append("%s: status is not 0 on %d arms" % (fam, int((got["status"] != 0).sum())))
        if fam == "pub":
            _check_v6(got["v6"], ref, io_dtype, R, "pub v6", sc, failures, row)
            if not np.array_equal(got["qdot_out"], got["qdot_vf"]):
                failures.append("pub: qdot_out differs from qdot_vf without a module flag")
        _check_qdot(got["qdot_out"], refq, ref, bar, io_dtype, fam + " qdot", sc, failures, row)
    if sid == "1-o5":   # the rollout: two cycles, the second from where the reference's first leaves the arms
        q1 = w["q"] + DT * (refq["qdot"] + refq["qdot_lo"])
        key2 = ("field-roll", np.dtype(io_dtype).name)
        ref2 = hf.reference(key2, w["fields"], w["nfields"], params.rot_slowdown, params.speed_scale, chain=chain, q=q1)
        refq2, Rs2 = _solve_refs(oc, sc, ref2, q1, key2, "field-roll")
        bar2 = _qdot_bar(refq2, ref2, io_dtype, R, max(Rs, Rs2))
        eng = engine.Engine(chain, hf.B_ARMS, io_dtype=io_dtype, max_slots=sc["max_slots"], params=params)
        try:
            eng.set_fields(w["fields"], w["nfields"])
            got = eng.rollout_host(w["q"], 2, DT, want=LEAN)
        finally:
            eng.close()
        q2 = q1 + DT * (refq2["qdot"] + refq2["qdot_lo"])
        qbar = DT * (bar + bar2) + (2.0 ** -24 * np.abs(q2) if io_dtype == np.float32 else 4 * hp.U * np.abs(q2))
        qerr = np.abs(got["q"].astype(np.float64) - q2)
        held = ~(ref["finite_only"] | ref2["finite_only"])
        over = np.where(held[:, None], qerr / qbar, 0.0)
        wb = int(np.argmax(over.max(axis=1)))
        print("    %-12s worst err / bar %.3f (arm %d %s: err %.3e)" % ("roll q", over.max(), wb, hf.kinds_of(sc, wb), qerr[wb].max()))
        row.append(("roll q", float(over.max()), hf.kinds_of(sc, wb), float(over.max())))
        if not (np.all(np.isfinite(got["q"])) and over.max() <= 1.0 and np.all(got["status"] == 0)):
            failures.append("roll: q after two cycles err / bar = %.2f on arm %d (%s)" % (over.max(), wb, hf.kinds_of(sc, wb)))
    _TABLE[(sid, np.dtype(io_dtype).name)] = (R, row)
    _write_table()
    assert not failures, "%d failures:\n" % len(failures) + "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("sid", hf.PROBE_SCENES)
def test_probe_kernel_against_the_field_reference(sid, io_dtype):
    oc, engine = _env()
    sc, ref, R = hf.oracle_scene(oc, sid, io_dtype)
    w = sc["w"]
    assert np.all(ref["kappa_pose"] == 0.0)
    print("\n%s %s: oracle err / E %.3f, max kappa_sum %.2e, max kappa_rel %.2e" % (sid, np.dtype(io_dtype).name, R, ref["kappa_sum"].max(), ref["kappa_rel"].max()))
    failures, row = [], []
    eng = engine.Engine(sc["chain"], hf.B_ARMS, io_dtype=io_dtype, max_slots=sc["max_slots"], params=sc["params"])
    try:
        eng.set_fields(w["fields"], w["nfields"])
        esz = np.dtype(io_dtype).itemsize
        d_pose, d_v6 = eng.dev_alloc(hf.B_ARMS * 16 * esz), eng.dev_alloc(hf.B_ARMS * 6 * esz)
        eng.h2d(d_pose, sc["pose"].astype(io_dtype))
        eng.probe_field(d_pose, d_v6)
        got = np.zeros((hf.B_ARMS, 6), dtype=io_dtype)
        eng.d2h(got, d_v6)
        eng.dev_free(d_pose)
        eng.dev_free(d_v6)
    finally:
        eng.close()
    _check_v6(got, ref, io_dtype, R, "probe v6", sc, failures, row)
    _TABLE[(sid, np.dtype(io_dtype).name)] = (R, row)
    _write_table()
    assert not failures, "%d failures:\n" % len(failures) + "\n".join(failures)
