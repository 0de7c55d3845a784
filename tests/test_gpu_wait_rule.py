"""Coupled goto_host and follow_host under a wait rule (include/vfik.h: vfik_set_wait_rule) on the GPU against tests/clearance_reference.py,
the oracle-stepped coupled move with the rule in front of every block.

The moves: goto64, goto32 and follow of coupled_reference.MOVES through pair_case, the ODD arms yielding, min_clearance per move from
clearance_reference.MIN_CLEARANCE -- chosen on the CPU so that in the ORACLE's run at least ten arms wait for a block or more and later
run again, at least one arm waits through the last block and at least half of the yielding arms never wait (asserted here on the
reference's run, and in tests/test_wait_reference.py).

Against the reference: waited, arrived / reached / next exact, the joint path within coupled_reference.PATH_BAR, clear_traj within the
kernel test's bar plus the path bar times the reach.  Left out of the exact comparison: the arms the suite leaves out already (within the
margin of an arrival threshold in the reference's run), the arms whose clearance in the reference's run comes within that margin of
min_clearance at any block, and the partners of both; the share is capped at 5 % (15 %) on the reference's numbers before the GPU's are
read.  pending is a count over the batch: exact where nobody is left out, else within the number of arms left out.
For EVERY arm, on the GPU's own rows: the state machine with the rule replayed on the GPU's clear_traj (the I/O-typed compare makes that
exact) gives the GPU's waited, arrived / reached / next and pending, and an arm the replay keeps out of a block repeats its row;
clear_traj[k] and pair_traj[k] equal link_clearance of q_traj[k - 1] and link_traj[k] bit for bit.
A rule under which no arm yields equals the coupled move without a rule bit for bit, and so does the move after the rule was switched off."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_reference as wr  # noqa: E402
import coupled_reference as cr  # noqa: E402
import hp_clearance as hc  # noqa: E402
import hp_links as hl  # noqa: E402
import timed_reference as tr  # noqa: E402

pytestmark = pytest.mark.gpu

N_CYCLES, DT, PREC = cr.N_CYCLES, cr.DT, cr.PREC
KEYS = ("q_traj", "dist_traj", "pending", "q", "qdot_out", "status")


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
    return e


def _engine(env, name, c, params, yields="odd", rule=True):
    m = cr.MOVES[name]
    n_checks = N_CYCLES // m["stride"]
    eng = env.engine.Engine(c["chain"], m["B"], io_dtype=m["io_dtype"], max_slots=8, params=params)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.set_link_spheres(c["spheres"])
    eng.set_coupling(src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"], trace_checks=n_checks)
    if rule:
        yl = wr.yields_of(m["B"]) if isinstance(yields, str) else yields
        eng.set_wait_rule(wr.MIN_CLEARANCE[name], yields=yl, trace_checks=n_checks)
    return eng


def _move(eng, name, c):
    m = cr.MOVES[name]
    q_in = c["q0"].astype(eng.io_dtype)
    common = dict(stride=m["stride"], hold=m["hold"], clamp=True, trajectory=True, want=("qdot_out", "status"))
    if c["way"] is None:
        return eng.goto_host(q_in, N_CYCLES, DT, PREC, **common)
    return eng.follow_host(q_in, c["way"], N_CYCLES, DT, PREC, **common)


def _outcome(c, r):
    return (r["arrived"],) if c["way"] is None else (r["reached"], r["next"])


def _replay(name, c, ref, got, clear):
    """The state machine and the rule on the GPU's own rows.  Returns (machine, waited (B,), kept_out (checks, B): who did not run)."""
    m = cr.MOVES[name]
    B, n = c["q0"].shape
    if c["way"] is None:
        kind, wayq = np.full((B, 1), tr.FRAME, dtype=np.int32), np.zeros((B, 1, n))
    else:
        kind, wayq = tr.list_kind(c["way"], tr.FRAME), np.zeros((B, c["way"].shape[1], n))
    mach = tr.Machine(kind, wayq, ref["present"], N_CYCLES, m["stride"], PREC, np.zeros(n), hold=m["hold"], io_dtype=m["io_dtype"])
    yl = wr.yields_of(B) != 0
    waited, kept_out = np.zeros(B, dtype=np.int32), np.zeros(clear.shape, dtype=bool)
    for k in range(clear.shape[0]):
        with np.errstate(invalid="ignore"):
            wait = mach.gate & yl & (clear[k].astype(np.float64) < wr.MIN_CLEARANCE[name])
        waited += wait
        mach.gate[wait] = False
        kept_out[k] = ~mach.gate
        mach.check(k, got["q_traj"][k].astype(np.float64), got["dist_traj"][k].astype(np.float64))
    return mach, waited, kept_out


@pytest.mark.parametrize("name", ["goto64", "goto32", "follow"])
def test_against_the_reference(env, name):
    c, params, ref = wr.reference(env.oc, name)
    m = cr.MOVES[name]
    B, io, L = m["B"], np.dtype(m["io_dtype"]), len(c["spheres"])
    n_checks = N_CYCLES // m["stride"]
    yl = wr.yields_of(B)
    # the scene and who is left out: on the reference's run, before the GPU's is read
    again, last, never = wr.conditions(ref, yl)
    print("%s: reference: %d arms wait and run again, %d wait through the last block, %.0f %% of the yielding arms never wait" % (name, again, last, 100 * never))
    assert again >= 10 and last >= 1 and never >= 0.5
    part = ref["length"] > 0
    near = wr.near_rule(ref, yl, wr.MIN_CLEARANCE[name], io)
    out, _near, share, cap = cr.left_out(ref, part, io, c["src_arm"], True, near)
    print("%s: left out %d of %d arms (%.1f %%, cap %.0f %%)" % (name, np.count_nonzero(out & part), np.count_nonzero(part), 100 * share, 100 * cap))
    assert share <= cap, share
    inc = ~out

    eng = _engine(env, name, c, params)
    got = _move(eng, name, c)
    clear, pair = eng.clearance_traj()
    link = eng.link_traj()
    assert got["checks_run"] == n_checks and clear.shape == (n_checks, B) and clear.dtype == io and pair.dtype == np.int32

    # against the reference
    assert np.array_equal(got["waited"][inc], ref["waited"][inc]), np.flatnonzero(inc & (got["waited"] != ref["waited"]))
    for a, b in zip(_outcome(c, got), _outcome(c, ref)):
        assert np.array_equal(a[inc], b[inc])
    slack = np.count_nonzero(out & part)
    assert np.all(np.abs(got["pending"] - ref["pending"]) <= slack), (got["pending"], ref["pending"])
    eq = np.abs(got["q_traj"][:, inc].astype(np.float64) - ref["q_traj"][:, inc])
    print("%s: q_traj max error %.3e (bar %.1e)" % (name, eq.max(), cr.PATH_BAR[io]))
    assert eq.max() < cr.PATH_BAR[io]
    reach = hl.reach(c["chain"], c["spheres"])
    with np.errstate(invalid="ignore"):
        # the kernel test's unit with a cap in place of the minimising pair's own numbers: |Q_j| + R_j <= 3 max |row element|
        rows = np.abs(ref["link_traj"]).max(axis=(2, 3))                                   # (checks, B)
        unit = c["chain"].n * hc.U * (reach.max() + 3.0 * np.where(np.isnan(rows), 0.0, rows) + max(s[2] for s in c["spheres"]))
        half_ulp = 0.5 * np.spacing(np.abs(np.where(np.isfinite(ref["clear_traj"]), ref["clear_traj"], 1.0)).astype(io)).astype(np.float64)
        bar = hc.K_MARGIN * unit + half_ulp + cr.PATH_BAR[io] * reach.max()
        d = np.abs(clear.astype(np.float64) - ref["clear_traj"])
    fin = np.isfinite(ref["clear_traj"])
    assert np.array_equal(np.isposinf(clear), np.isposinf(ref["clear_traj"]))
    print("%s: clear_traj max error %.3e (smallest bar %.3e)" % (name, d[fin & inc[None, :]].max(), bar[fin & inc[None, :]].min()))
    assert np.all(d[fin & inc[None, :]] <= bar[fin & inc[None, :]])

    # every arm, on the GPU's own rows
    mach, waited, kept_out = _replay(name, c, ref, got, clear)
    assert np.array_equal(got["waited"], waited)
    if c["way"] is None:
        assert np.array_equal(got["arrived"], mach.reached[:, 0])
    else:
        assert np.array_equal(got["reached"], mach.reached) and np.array_equal(got["next"], mach.next)
    assert np.array_equal(got["pending"], mach.pending)
    q_in = np.concatenate([c["q0"].astype(io)[None], got["q_traj"][:-1]], axis=0)
    assert np.all(got["q_traj"][kept_out] == q_in[kept_out])                              # the gate: who is kept out repeats its row
    moved = np.any(got["q_traj"] != q_in, axis=2)
    assert not np.any(moved & kept_out) and np.count_nonzero(moved & ~kept_out) > 0
    for k in range(n_checks):
        want_c, want_p = eng.link_clearance_host(q_in[k].astype(np.float64), link[k].astype(np.float64), 0, L)
        assert np.array_equal(clear[k].astype(np.float64), want_c) and np.array_equal(pair[k], want_p), k
    # an arm that waited through block 0 and the host form's rows: its q row is the caller's
    w0 = (got["waited"] > 0) & kept_out[0] & (yl != 0) & part
    assert np.all(got["q_traj"][0, w0] == c["q0"].astype(io)[w0])
    eng.close()


@pytest.mark.parametrize("name", ["goto64", "goto32"])
def test_nobody_yields_and_rule_off_equal_the_coupled_move(env, name):
    c, params, _ref = cr.reference(env.oc, name)
    B = cr.MOVES[name]["B"]
    keys = KEYS + ("arrived",)
    plain = _engine(env, name, c, params, rule=False)
    want = _move(plain, name, c)
    want_link = plain.link_traj()
    assert "waited" not in want
    # a rule under which no arm yields: the measurement runs before every block, nobody waits
    none = _engine(env, name, c, params, yields=np.zeros(B, dtype=np.int32))
    got = _move(none, name, c)
    assert all(np.array_equal(got[k], want[k]) for k in keys) and np.array_equal(none.link_traj(), want_link, equal_nan=True)
    assert not got["waited"].any() and np.isfinite(none.clearance_traj()[0][:, :B - 1]).all()
    # a move under the rule, then the rule off and the scene as it was: the coupled move
    eng = _engine(env, name, c, params)
    moved = _move(eng, name, c)
    assert moved["waited"].any() and not np.array_equal(moved["q_traj"], want["q_traj"])
    eng.set_wait_rule(None)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.reset_state()
    again = _move(eng, name, c)
    assert "waited" not in again and all(np.array_equal(again[k], want[k]) for k in keys)
    with pytest.raises(env.engine.VfikError):
        eng.waited()
    for e in (plain, none, eng):
        e.close()


def test_the_rule_goes_with_the_coupling(env):
    name = "goto32"
    c, params, _ref = cr.reference(env.oc, name)
    m = cr.MOVES[name]
    eng = env.engine.Engine(c["chain"], m["B"], io_dtype=m["io_dtype"], max_slots=8, params=params)
    eng.set_fields(c["w"]["fields"], c["w"]["nfields"])
    eng.set_link_spheres(c["spheres"])
    with pytest.raises(env.engine.VfikError, match="vfik_set_coupling"):
        eng.set_wait_rule(0.05)
    eng.set_coupling(src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])
    for bad in (dict(min_clearance=np.inf), dict(min_clearance=np.nan), dict(min_clearance=0.05, mask=[1 << len(c["spheres"])] * len(c["spheres"]))):
        with pytest.raises(env.engine.VfikError):
            eng.set_wait_rule(**bad)
    eng.set_wait_rule(0.05, yields=wr.yields_of(m["B"]))
    assert not eng.waited().any()                      # nobody waited before the first timed move
    for drop in (lambda: eng.set_coupling(None), lambda: eng.set_link_spheres(c["spheres"])):
        drop()
        with pytest.raises(env.engine.VfikError):
            eng.waited()
        eng.set_link_spheres(c["spheres"])
        eng.set_coupling(src_arm=c["src_arm"], xform=c["xform"], first_rep=c["first_rep"])
        eng.set_wait_rule(0.05)
    eng.close()
