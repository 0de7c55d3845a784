"""All five timed moves on the GPU with every rule of the handle switched on at once -- coupling + wait rule + avoid rule + stall rule, `stop`
and `hold` on -- against tests/rules_reference.py, the three wrappers of the suite stacked around the oracle in the device's order.

The scenes and moves: rules_reference.ALL -- coupled_reference.pair_case at 131 arms (the LWR; float64 at stride 1, float32 at stride 4)
and 67 arms (two LWRs in series, the stepped path; float64, stride 4), the odd arms yielding, every eighth arm's goal, frames and postures
out of reach, nullspace module and mixer with mix_w[4] = 1; goto, follow (W = 3), goto_js, follow_js (W = 3), the scripts P F F P and
F P F with arms whose scripts end early and one arm without one, and a script P F F with the rule on channel 3, whose weight is the
script's own rows'.  The scene conditions (rules_reference.conditions) are asserted on the REFERENCE's run before the GPU's rows are read.

Against the reference: waited, stalled, arrived / reached / next and way_traj exact, pending within the number of arms left out, the joint
path within coupled_reference.PATH_BAR (the bars of tests/test_gpu_goto_js.py are the same two numbers), diff within twice that and, where
the paths are equal, bit for bit.  Left out of the exact comparison (rules_reference.left_out): the arms within coupled_reference.MARGIN of an arrival threshold, of min_clearance or
of a stall eps step in the reference's run, and the arms they are the source of; capped at 5 % (float64) and 15 % (float32).

For EVERY arm, on the GPU's own rows: the state machine replayed with the wait rule on the GPU's clear_traj and the stall rule on its
dist_traj / q_traj gives the GPU's waited, stalled, arrivals, way_traj, pending and diff (bit for bit); an arm the replay keeps out of a
block repeats its rows; clear_traj[k] / pair_traj[k] equal link_clearance, avoid_traj[k] equals link_avoid -- for the arms that waited in
block k too -- and link_traj[k] equals link_points of q_traj[k - 1], all bit for bit.

Identities, bit for bit: nobody yields + scale zero + no stall rule is the coupled move; the rules switched off again is a handle that never
had them; the device-pointer forms equal the host forms; a second move on the same handle equals the move on a fresh one.  Early exit:
checks_run under poll=2 is what the reference's pending predicts, and the avoid channel is zero after a move that ended early.

With VFIK_RULES_TABLE=<file> the measured figures are also written there (the record kept in profiles/rules_together.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coupled_reference as cr  # noqa: E402
import rules_reference as rr  # noqa: E402
import timed_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

N_CYCLES, DT, PREC = cr.N_CYCLES, cr.DT, cr.PREC
KEYS = ("q_traj", "pending", "q", "qdot_out", "status", "waited", "stalled")
ALL = rr.ALL
IDS = ["%s-%s" % sm for sm in ALL]


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, engine
    oracle_c.build()

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine = oracle_c, _abi, engine
    e.table = {}
    yield e
    path = os.environ.get("VFIK_RULES_TABLE")
    if path and e.table:
        with open(path, "a") as f:
            for key in sorted(e.table):
                f.write("%-22s %s\n" % ("%s %s" % key, "; ".join(e.table[key])))


def _engine(env, c, params, wait=True, avoid=True, stall=True, coupled=True, yields=None, scale=None):
    s = rr.SCENES[c["scene"]]
    n_checks = N_CYCLES // s["stride"]
    eng = env.engine.Engine(c["chain"], s["B"], io_dtype=s["io_dtype"], max_slots=8, params=params)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    if coupled:
        eng.set_link_spheres(c["spheres"])
        eng.set_coupling(src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"], trace_checks=n_checks)
    t = rr.tuned(c["scene"], c["move"])
    if wait:
        eng.set_wait_rule(t["min_clearance"], yields=rr.yields_of(s["B"]) if yields is None else yields, trace_checks=n_checks)
    if avoid:
        a = t["avoid"]
        eng.set_avoid_rule(a["gain"], a["d0"], channel=rr.channel_of(c["move"]), scale=scale, trace_checks=n_checks)
    if stall:
        eng.set_stall_rule(**t["rule"])
    return eng


def _js(c):
    s, n = rr.SCENES[c["scene"]], c["chain"].n
    return np.full(n, s["js_prec"][0]), np.full(n, s["js_prec"][1])


def _mixes(c):
    ch3 = c["move"] == "script_ch3"
    return (rr.MIX_FRAME_CH3 if ch3 else rr._abi.MIX_FRAME), (rr.MIX_POSTURE_CH3 if ch3 else rr._abi.MIX_POSTURE)


def _move(eng, c, poll=0, n_cycles=N_CYCLES):
    s, move = rr.SCENES[c["scene"]], c["move"]
    io = eng.io_dtype
    q_in = c["q0"].astype(io)
    prec, via = _js(c)
    common = dict(stride=s["stride"], hold=True, clamp=True, trajectory=True, want=("qdot_out", "status"), poll=poll)
    if move == "goto":
        return eng.goto_host(q_in, n_cycles, DT, PREC, **common)
    if move == "follow":
        return eng.follow_host(q_in, c["way"], n_cycles, DT, PREC, **common)
    if move == "goto_js":
        return eng.goto_js_host(q_in, c["q_ref"].astype(io), n_cycles, DT, prec, **common)
    if move == "follow_js":
        return eng.follow_js_host(q_in, c["wayq"], n_cycles, DT, prec, via_precision=via, **common)
    mf, mp = _mixes(c)
    return eng.script_host(q_in, c["kind"], c["way_s"], c["wayq_s"], n_cycles, DT, PREC, prec, js_via_precision=via, mix_frame=mf, mix_posture=mp,
                           **common)


def _outcome(c, r):
    return ("arrived",) if c["move"] in ("goto", "goto_js") else ("reached", "next", "way_traj")


def _machine(c, present, n_cycles=N_CYCLES):
    """the state machine of the case's move, with the stall rule: what tests/timed_reference.py's forms hand to Machine"""
    s, move = rr.SCENES[c["scene"]], c["move"]
    B, n = c["q0"].shape
    prec, via = _js(c)
    pc, js, jv = PREC, np.zeros(n), None
    if move == "goto":
        kind, wayq = np.full((B, 1), tr.FRAME, dtype=np.int32), np.zeros((B, 1, n))
    elif move == "follow":
        kind, wayq = tr.list_kind(c["way"], tr.FRAME), np.zeros((B, c["way"].shape[1], n))
    elif move == "goto_js":
        kind, wayq, pc, js = np.full((B, 1), tr.POSTURE, dtype=np.int32), c["q_ref"][:, None, :], (0.0, 0.0), prec
    elif move == "follow_js":
        kind, wayq, pc, js, jv = tr.list_kind(c["wayq"], tr.POSTURE), c["wayq"], (0.0, 0.0), prec, via
    else:
        kind, wayq, js, jv = c["kind"], c["wayq_s"], prec, via
    return tr.Machine(kind, wayq, present, n_cycles, s["stride"], pc, js, None, jv, hold=True, io_dtype=s["io_dtype"],
                      rule=tr.Rule(**rr.tuned(c["scene"], move)["rule"]))


def _replay(c, present, got, clear):
    """The state machine, the wait rule and the stall rule on the GPU's own rows.  Returns (machine, waited (B,), kept_out (checks, B): who did
    not run, waits (checks, B): who of them waited)."""
    B = c["q0"].shape[0]
    mach = _machine(c, present)
    yl = rr.yields_of(B) != 0
    done = got["q_traj"].shape[0]
    waited, kept_out, waits = np.zeros(B, dtype=np.int32), np.zeros((done, B), dtype=bool), np.zeros((done, B), dtype=bool)
    for k in range(done):
        with np.errstate(invalid="ignore"):
            wait = mach.gate & yl & (clear[k].astype(np.float64) < rr.r_min(c))
        waited += wait
        mach.gate[wait] = False
        kept_out[k], waits[k] = ~mach.gate, wait
        dist = got["dist_traj"][k].astype(np.float64) if "dist_traj" in got else np.full((B, 2), np.nan)
        mach.check(k, got["q_traj"][k].astype(np.float64), dist)
    return mach, waited, kept_out, waits


def _same(a, b, keys):
    for k in keys:
        if k in a or k in b:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("scene,move", ALL, ids=IDS)
def test_against_the_reference_and_on_its_own_rows(env, scene, move):
    c, params, ref = rr.reference(env.oc, scene, move)
    s = rr.SCENES[scene]
    B, io, L, n = s["B"], np.dtype(s["io_dtype"]), len(c["spheres"]), c["chain"].n
    n_checks = N_CYCLES // s["stride"]
    yl = rr.yields_of(B) != 0
    # the scene and who is left out: on the reference's run, before the GPU's is read
    cond = rr.conditions(c, ref)
    print("%s %s: reference: %s" % (scene, move, cond))
    assert rr.conditions_hold(cond, B), cond
    out, part, share, cap = rr.left_out(c, ref)
    print("%s %s: left out %d of %d arms (%.1f %%, cap %.0f %%)" % (scene, move, np.count_nonzero(out & part), np.count_nonzero(part), 100 * share, 100 * cap))
    assert share <= cap, share
    inc = ~out
    slack = np.count_nonzero(out & part)

    eng = _engine(env, c, params)
    got = _move(eng, c)
    clear, pair = eng.clearance_traj()
    cmd, link = eng.avoid_traj(), eng.link_traj()
    assert got["checks_run"] == n_checks and clear.shape == (n_checks, B) and cmd.shape == (n_checks, B, n) and cmd.dtype == io

    # against the reference
    for k in ("waited", "stalled") + _outcome(c, ref):
        a, b = (got[k], ref[k]) if k != "way_traj" else (got[k].T, ref[k].T)
        assert np.array_equal(a[inc], b[inc]), (k, np.flatnonzero(inc & np.any((a != b).reshape(B, -1), axis=1)))
    assert np.all(np.abs(got["pending"].astype(np.int64) - ref["pending"]) <= slack), (got["pending"], ref["pending"])
    eq = np.abs(got["q_traj"][:, inc].astype(np.float64) - ref["q_traj"][:, inc])
    print("%s %s: q_traj max error %.3e (bar %.1e)" % (scene, move, eq.max(), cr.PATH_BAR[io]))
    for b in np.flatnonzero(inc)[np.flatnonzero(eq.max(axis=(0, 2)) >= cr.PATH_BAR[io])][:8]:   # (what a failure is read from)
        e = np.abs(got["q_traj"][:, b].astype(np.float64) - ref["q_traj"][:, b]).max(axis=1)
        k = int(np.argmax(e >= cr.PATH_BAR[io]))
        print("  arm %d (source %d): over the bar from check %d (%.2e; the check before %.2e), at the end %.2e; waited %d, stalled %d, "
              "largest command %.2e, smallest clearance %.4f" % (b, c["src_arm"][b], k, e[k], e[max(k - 1, 0)], e[-1], got["waited"][b], got["stalled"][b],
                                                                 np.abs(cmd[:, b]).max(), np.nanmin(clear[:, b].astype(np.float64))))
    assert eq.max() < cr.PATH_BAR[io]
    if "diff" in got:
        # diff = (T)(ref - q) of an arm's last posture check: bit for bit against the reference's where the paths are equal (float32: they
        # are), else within the two roundings a path inside its bar can move it by; bit for bit on the GPU's own rows below, every arm
        ed = np.abs(got["diff"][inc].astype(np.float64) - ref["diff"][inc])
        assert ed[~np.isnan(ed)].max() < 2 * cr.PATH_BAR[io]
        if eq.max() == 0.0:
            assert np.array_equal(got["diff"][inc].astype(np.float64), ref["diff"][inc], equal_nan=True)

    # every arm, on the GPU's own rows: the machine with both rules replayed
    mach, waited, kept_out, waits = _replay(c, ref["present"], got, clear)
    assert np.array_equal(got["waited"], waited) and np.array_equal(got["stalled"], mach.stalled)
    if "arrived" in got:
        assert np.array_equal(got["arrived"], mach.reached[:, 0])
    else:
        assert np.array_equal(got["reached"], mach.reached) and np.array_equal(got["next"], mach.next)
        assert np.array_equal(got["way_traj"], mach.way_traj)
    assert np.array_equal(got["pending"], mach.pending)
    if "diff" in got:
        assert got["diff"].dtype == io and np.array_equal(got["diff"], mach.diff, equal_nan=True)
    q_in = np.concatenate([c["q0"].astype(io)[None], got["q_traj"][:-1]], axis=0)
    assert np.all(got["q_traj"][kept_out] == q_in[kept_out])                              # who is kept out of a block repeats its row
    if "dist_traj" in got:
        d_in = got["dist_traj"][:-1]
        assert np.array_equal(got["dist_traj"][1:][kept_out[1:]], d_in[kept_out[1:]], equal_nan=True)
    moved = np.any(got["q_traj"] != q_in, axis=2)
    assert not np.any(moved & kept_out) and np.count_nonzero(moved & ~kept_out) > 0
    gain, d0 = rr.tuned(scene, move)["avoid"]["gain"], rr.tuned(scene, move)["avoid"]["d0"]
    for k in range(n_checks):
        qk, lk = q_in[k].astype(np.float64), link[k].astype(np.float64)
        assert np.array_equal(lk, eng.link_points_host(qk, c["src_arm"], c["xform"]), equal_nan=True), k
        want_c, want_p = eng.link_clearance_host(qk, lk, 0, L)
        assert np.array_equal(clear[k].astype(np.float64), want_c) and np.array_equal(pair[k], want_p), k
        assert np.array_equal(cmd[k].astype(np.float64), eng.link_avoid_host(qk, lk, 0, L, gain=gain, d0=d0)), k
    # the command of an arm that waits is computed and traced, and never taken
    assert waits.any() and np.any(cmd[waits] != 0) and not np.any(moved & waits)
    # an arm that waits through the last block keeps pending up; a stalled arm is not in it
    under_way = (mach.L > 0) & (mach.next < mach.L) & (mach.stalled < 0)
    assert np.all(under_way[waits[-1]]) and got["pending"][-1] == np.count_nonzero(under_way)
    # the poll: checks_run under poll=2 is what the reference's pending predicts -- a waiting arm keeps it up, a stalled arm does not
    zero = np.flatnonzero((ref["pending"][1::2] == 0) & (np.arange(2, n_checks + 1, 2) < n_checks))
    predicted = int(2 * (zero[0] + 1)) if len(zero) else n_checks
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.reset_state()
    early = _move(eng, c, poll=2)
    if slack == 0:
        assert early["checks_run"] == predicted, (early["checks_run"], predicted)
    own = np.flatnonzero((got["pending"][1::2] == 0) & (np.arange(2, n_checks + 1, 2) < n_checks))
    assert early["checks_run"] == (int(2 * (own[0] + 1)) if len(own) else n_checks)
    _same(early, {k: (v[:early["checks_run"]] if k in ("q_traj", "pending") else v) for k, v in got.items()}, ("q_traj", "pending"))
    env.table[(scene, move)] = ["%s" % " ".join("%s %d" % kv for kv in cond.items() if kv[0] != "far_arms"),
                                "left out %.1f %% (cap %.0f %%)" % (100 * share, 100 * cap),
                                "path error %.2e (bar %.0e)" % (eq.max(), cr.PATH_BAR[io]),
                                "checks_run under poll=2: %d of %d (predicted %d)" % (early["checks_run"], n_checks, predicted)]
    eng.close()


IDENT = ALL            # the identities compare the GPU with itself: every scene and move


@pytest.mark.parametrize("scene,move", IDENT, ids=["%s-%s" % sm for sm in IDENT])
def test_rules_that_do_nothing_and_rules_switched_off_equal_the_coupled_move(env, scene, move):
    c, params, _ref = rr.reference(env.oc, scene, move)
    B = rr.SCENES[scene]["B"]
    keys = tuple(k for k in KEYS if k not in ("waited", "stalled")) + ("arrived", "reached", "next", "way_traj", "dist_traj", "diff")
    plain = _engine(env, c, params, wait=False, avoid=False, stall=False)
    want = _move(plain, c)
    want_link = plain.link_traj()
    assert "waited" not in want and "stalled" not in want
    # nobody yields, nobody gives way, no stall rule: the kernels run in front of every block and change nothing
    none = _engine(env, c, params, stall=False, yields=np.zeros(B, dtype=np.int32), scale=np.zeros(B))
    got = _move(none, c)
    assert not got["waited"].any() and not none.avoid_traj().any()
    _same(got, want, keys)
    assert np.array_equal(none.link_traj(), want_link, equal_nan=True)
    # a move under all the rules, then the rules off and the scene as it was: a handle that never had them
    eng = _engine(env, c, params)
    moved = _move(eng, c)
    assert moved["waited"].any() and (moved["stalled"] >= 0).any() and eng.avoid_traj().any() and not np.array_equal(moved["q_traj"], want["q_traj"])
    eng.set_wait_rule(None)
    eng.set_avoid_rule(None)
    eng.set_stall_rule(None)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.reset_state()
    again = _move(eng, c)
    assert "waited" not in again and "stalled" not in again
    _same(again, want, keys)
    for e in (plain, none, eng):
        e.close()


@pytest.mark.parametrize("scene,move", IDENT, ids=["%s-%s" % sm for sm in IDENT])
def test_a_second_move_equals_the_move_on_a_fresh_handle(env, scene, move):
    """`waited`, the stall state and the avoid channel are all reset by the next move: the same move again -- the scene put back and the
    module states reset, the rules untouched -- gives the first move's arrays and traces, which are a fresh handle's"""
    c, params, _ref = rr.reference(env.oc, scene, move)
    eng = _engine(env, c, params)
    first = _move(eng, c)
    traces = (eng.clearance_traj(), eng.avoid_traj(), eng.link_traj())
    assert first["waited"].any() and (first["stalled"] >= 0).any()
    # something else in between, cut short: its waited, stall state and channel must not leak
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.reset_state()
    _move(eng, c, n_cycles=N_CYCLES // 2)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.reset_state()
    second = _move(eng, c)
    _same(second, first, KEYS + ("arrived", "reached", "next", "way_traj", "dist_traj", "diff"))
    again = (eng.clearance_traj(), eng.avoid_traj(), eng.link_traj())
    assert np.array_equal(again[0][0], traces[0][0]) and np.array_equal(again[0][1], traces[0][1])
    assert np.array_equal(again[1], traces[1]) and np.array_equal(again[2], traces[2], equal_nan=True)
    eng.close()


@pytest.mark.parametrize("scene,move", IDENT, ids=["%s-%s" % sm for sm in IDENT])
def test_device_form_equals_host_form(env, scene, move):
    """Engine.goto .. Engine.script on torch tensors under all the rules give the host forms' arrays and traces"""
    import torch
    c, params, _ref = rr.reference(env.oc, scene, move)
    s = rr.SCENES[scene]
    B, io, n, stride = s["B"], np.dtype(s["io_dtype"]), c["chain"].n, s["stride"]
    n_checks = N_CYCLES // stride
    eng = _engine(env, c, params)
    host = _move(eng, c)
    host_tr = (eng.clearance_traj(), eng.avoid_traj(), eng.link_traj())
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.reset_state()
    dev = torch.device("cuda", 0)
    ft = torch.float64 if io == np.float64 else torch.float32

    def t(a, dtype=None):
        return torch.from_numpy(np.array(a, dtype=dtype or io, order="C")).to(dev)
    q, qd = t(c["q0"]), torch.zeros(B, n, dtype=ft, device=dev)
    o = dict(pending=torch.zeros(n_checks, dtype=torch.int32, device=dev), q_out=torch.zeros(B, n, dtype=ft, device=dev),
             q_traj=torch.zeros(n_checks, B, n, dtype=ft, device=dev))
    prec, via = _js(c)
    kw = dict(stride=stride, hold=True, clamp=True)
    W = {"follow": rr.W, "follow_js": rr.W}.get(move, len(rr.SCRIPTS.get(move, "x")))
    if move in ("goto", "goto_js"):
        o["arrived"] = torch.full((B,), -1, dtype=torch.int32, device=dev)
    else:
        o["reached"], o["next"] = torch.full((B, W), -1, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        o["way_traj"] = torch.full((n_checks, B), -1, dtype=torch.int32, device=dev)
    if move in ("goto", "follow") or move in rr.SCRIPTS:
        o["dist_traj"] = torch.zeros(n_checks, B, 2, dtype=ft, device=dev)
    if move not in ("goto", "follow"):
        o["diff"] = torch.zeros(B, n, dtype=ft, device=dev)
    torch.cuda.synchronize()
    if move == "goto":
        eng.goto(eng.make_io(q, qdot_out=qd), N_CYCLES, DT, PREC, **kw, **o)
    elif move == "follow":
        eng.follow(eng.make_io(q, qdot_out=qd), t(c["way"]), N_CYCLES, DT, PREC, **kw, **o)
    elif move == "goto_js":
        eng.goto_js(eng.make_io(q, q_ref=t(c["q_ref"]), qdot_out=qd), N_CYCLES, DT, prec, **kw, **o)
    elif move == "follow_js":
        eng.follow_js(eng.make_io(q, qdot_out=qd), t(c["wayq"]), N_CYCLES, DT, prec, via_precision=via, **kw, **o)
    else:
        mf, mp = _mixes(c)
        eng.script(eng.make_io(q, qdot_out=qd), t(c["kind"], np.int32), t(c["way_s"]), t(c["wayq_s"]), N_CYCLES, DT, PREC, prec,
                   js_via_precision=via, mix_frame=mf, mix_posture=mp, **kw, **o)
    eng.sync()
    for k, v in o.items():
        assert np.array_equal(v.cpu().numpy(), host["q" if k == "q_out" else k], equal_nan=True), k
    assert np.array_equal(qd.cpu().numpy(), host["qdot_out"])
    assert np.array_equal(eng.waited(), host["waited"]) and np.array_equal(eng.stalled(), host["stalled"])
    dev_tr = (eng.clearance_traj(), eng.avoid_traj(), eng.link_traj())
    assert np.array_equal(dev_tr[0][0], host_tr[0][0]) and np.array_equal(dev_tr[0][1], host_tr[0][1])
    assert np.array_equal(dev_tr[1], host_tr[1]) and np.array_equal(dev_tr[2], host_tr[2], equal_nan=True)
    eng.close()


def test_stalled_arms_let_the_poll_end_the_move_and_the_channel_is_zero_afterwards(env):
    """Nobody yields (so nobody waits): every arm arrives or stalls, pending reaches 0 and poll=2 ends the move where the reference's
    pending says.  After that early end the avoid channel is zero: the next step is that of a handle whose channel was zeroed."""
    scene, move = rr.POLL_CASE
    c, params, ref = rr.poll_reference(env.oc)
    s = rr.SCENES[scene]
    B, n_checks = s["B"], rr.POLL_CYCLES // s["stride"]
    out, part, share, cap = rr.left_out(c, ref)
    zero = np.flatnonzero((ref["pending"][1::2] == 0) & (np.arange(2, n_checks + 1, 2) < n_checks))
    assert share <= cap and len(zero) and (ref["stalled"] >= 0).sum() >= 4, (share, ref["pending"])
    predicted = int(2 * (zero[0] + 1))
    eng = _engine(env, c, params, yields=np.zeros(B, dtype=np.int32))
    got = _move(eng, c, poll=2, n_cycles=rr.POLL_CYCLES)
    print("checks_run %d of %d, predicted %d; %d stalled" % (got["checks_run"], n_checks, predicted, (got["stalled"] >= 0).sum()))
    if not np.any(out & part):
        assert got["checks_run"] == predicted
    assert got["checks_run"] < n_checks and got["pending"][-1] == 0 and (got["stalled"] >= 0).sum() >= 4
    assert eng.avoid_traj()[got["checks_run"] - 1].any()                      # the last block that ran did push
    q = got["q"].astype(np.float64)
    eng.reset_state()
    a = eng.step_host(q, want=("qdot_out",))["qdot_out"]
    eng.set_avoid_rule(None)
    eng.set_ext_cmd(rr.channel_of(move), None)
    eng.reset_state()
    b = eng.step_host(q, want=("qdot_out",))["qdot_out"]
    assert np.array_equal(a, b)
    eng.set_ext_cmd(rr.channel_of(move), np.full((B, c["chain"].n), 0.01))    # (and the channel does reach qdot_out)
    eng.reset_state()
    assert not np.array_equal(eng.step_host(q, want=("qdot_out",))["qdot_out"], b)
    env.table[(scene, move + " poll")] = ["nobody yields: checks_run under poll=2: %d of %d (predicted %d), %d stalled" % (
        got["checks_run"], n_checks, predicted, (got["stalled"] >= 0).sum())]
    eng.close()
