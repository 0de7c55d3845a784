"""The host-pointer call forms (vfik_step_host, vfik_rollout_host, vfik_submit_host, vfik_goto_host and the two move forms) through
every branch of their staging: the three of vfik_step_host -- the kernels on the pinned arena itself, one arena with one copy each way,
a device buffer and a copy per member --, each against vfik_step on device pointers (bit for bit: the same kernel on the same inputs)
and against the CPU oracle; the fresh-q gate in each of them (gated rows come back as they went in); the rollout's q; the pipelined
form from pinned and from pageable arrays; and what the forms' grown-on-demand buffers add to vfik_device_bytes.

LWR chain, 2 repellers, nullspace + mixer.  The shapes follow from the thresholds of cycles_host (vfclik_amd/csrc/vfik_abi.cpp) and are
re-derived in `_branch` below, so that a shape which no longer reaches its branch fails here instead of passing on another one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLOAT_OUTS = ("qdot_vf", "qdot_null", "qdot_out", "pose", "pose_nt", "v6", "qdist")   # what the oracle computes, beside status
EVERY_OUT = FLOAT_OUTS + ("status", "goal_dist", "q_ref_out", "track_error", "obj_dist")
SENTINEL = -777.25


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle_c
    from vfclik_amd import _abi, engine, robots, synth

    class E:
        pass

    e = E()
    e.oc, e.abi, e.engine, e.synth = oracle_c, _abi, engine, synth
    e.chain = robots.lwr()
    e.params = _abi.default_params(flags=_abi.F_NULLSPACE | _abi.F_MIXER)
    e.cache = {}
    return e


def _workload(env, B, dt):
    """Inputs of a case and the oracle's outputs for them, computed once per (B, dtype)."""
    if (B, dt) not in env.cache:
        w = env.synth.make_workload(env.chain, B, 2, seed=B, io_dtype=dt)
        rng = np.random.default_rng(B + 1)
        w["q"] = w["q"].astype(dt)
        w["ctrl"] = rng.uniform(-1, 1, (B, 4)).astype(dt)
        w["q_ref"] = np.clip(w["q"] + 0.1 * rng.normal(size=w["q"].shape), env.chain.q_lo, env.chain.q_hi).astype(dt)
        w["objects"] = env.chain.fk(rng.uniform(env.chain.q_lo, env.chain.q_hi, (B * 2, 7))).reshape(B, 2, 16)
        w["gate"] = (np.arange(B) % 3 != 0).astype(np.int32)   # every third arm silent
        w["oracle"] = {}
        env.cache[(B, dt)] = w
    return env.cache[(B, dt)]


def _oracle(env, w, members):
    """The CPU oracle's cycle for the inputs of `members`.  q_ref: the joint controller's channel has mixer weight 0 here, what it adds
    is its status bit (oracle_c.joint_p)."""
    key = tuple(members[0])
    if key not in w["oracle"]:
        q = w["q"].astype(np.float64)
        ref = env.oc.cycle_batch(env.chain, env.params, q, w["fields"], w["nfields"],
                                 null_control=w["ctrl"].astype(np.float64) if "ctrl" in key else None)
        if "q_ref" in key:
            _, at_goal = env.oc.joint_p(w["q_ref"].astype(np.float64), q, env.chain.q_lo, env.chain.q_hi, env.params.jp_kp, env.params.jp_delta)
            ref["status"] = ref["status"] | np.where(at_goal != 0, env.abi.ST_JOINT_AT_GOAL, 0).astype(np.int32)
        w["oracle"][key] = ref
    return w["oracle"][key]


def _engine(env, w, dt):
    eng = env.engine.Engine(env.chain, w["q"].shape[0], io_dtype=dt, max_slots=4, params=env.params)
    eng.set_fields(w["fields"], w["nfields"])
    eng.set_objects(w["objects"])
    return eng


# the members of the three cases: inputs (beside the gate) and outputs
FULL = (("q", "ctrl", "q_ref"), EVERY_OUT)
LEAN = (("q",), ("qdot_out",))
CASES = {   # branch: B for float64, B for float32, members
    "zero_copy": (37, 37, FULL),
    "arena": (700, 700, FULL),
    "per_member": (5000, 9000, LEAN),   # (float32: three members of 5 000 arms stay under the bar of 512 KiB)
}
IN_NAMES = {"q": "q", "ctrl": "null_control", "q_ref": "q_ref"}


def _branch(B, dt, members, gated):
    """Which branch of cycles_host a call of these members takes: its own arithmetic, restated."""
    esz, n = np.dtype(dt).itemsize, 7
    cols = {"q": n, "ctrl": 4, "q_ref": n, "qdot_vf": n, "qdot_null": n, "qdot_out": n, "pose": 16, "pose_nt": 16, "v6": 6, "qdist": n,
            "goal_dist": 2, "q_ref_out": n, "track_error": 8, "obj_dist": 4}
    names = list(members[0]) + list(members[1])
    sizes = [B * 4 if k == "status" else B * cols[k] * esz for k in names] + ([B * 4] if gated else [])
    total = sum((s + 255) // 256 * 256 for s in sizes)
    if total > (256 << 10) and total > max(0, len(sizes) - 2) * (512 << 10):
        return "per_member"
    return "zero_copy" if total <= (64 << 10) else "arena"


def _host_step(env, eng, w, members, active=None, into=None):
    ins = {IN_NAMES[k]: w[k] for k in members[0]}
    return eng.step_host(want=members[1], active=active, into=into, **ins)


def _device_step(eng, w, members, dt, active=None):
    """vfik_step on device pointers: the same members, copied in and out one by one around the launch."""
    held, ins, outs, host = [], {}, {}, {}

    def dev(arr):
        p = eng.dev_alloc(arr.nbytes)
        held.append(p)
        eng.h2d(p, arr)
        return p

    for k in members[0]:
        ins[IN_NAMES[k]] = dev(np.ascontiguousarray(w[k], dtype=dt))
    if active is not None:
        ins["active"] = dev(np.ascontiguousarray(active, dtype=np.int32))
    for k in members[1]:
        shape, kdt = eng._out_spec(k)
        host[k] = np.zeros(shape, dtype=kdt)
        outs[k] = dev(host[k])
    eng.step(eng.make_io(**ins, **outs))
    eng.sync()
    for k in members[1]:
        eng.d2h(host[k], outs[k])
    for p in held:
        eng.dev_free(p)
    return host


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("branch", list(CASES))
def test_step_host_branch_equals_device_pointers_and_oracle(env, branch, dt):
    B64, B32, members = CASES[branch]
    B = B64 if dt == np.float64 else B32
    gate_all = branch == "per_member"   # (its three members: q, active, qdot_out -- a gate of ones)
    assert _branch(B, dt, members, gate_all) == branch
    w = _workload(env, B, dt)
    active = np.ones(B, dtype=np.int32) if gate_all else None
    eng = _engine(env, w, dt)
    got = _host_step(env, eng, w, members, active=active)
    eng.close()
    eng = _engine(env, w, dt)
    dev = _device_step(eng, w, members, dt, active=active)
    eng.close()
    for k in members[1]:
        assert got[k].tobytes() == dev[k].tobytes(), "%s: the host form and vfik_step on device pointers differ" % k
    tol = 1e-9 if dt == np.float64 else 2e-5
    ref = _oracle(env, w, members)
    for k in members[1]:
        if k in FLOAT_OUTS:
            err = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
            print("%s %s B=%d %-9s max|hip - oracle| = %.3e" % (branch, np.dtype(dt).name, B, k, err))
            assert err < tol, (k, err)
    if "status" in members[1]:
        print("status differs at arms", np.nonzero(got["status"] != ref["status"])[0][:8])
        assert np.array_equal(got["status"], ref["status"])
    if "obj_dist" in members[1]:   # (not the oracle's: that they were computed at all)
        assert np.all(got["goal_dist"][:, 0] > 0) and np.all(got["obj_dist"][:, :, 0] > 0) and np.all(np.abs(got["q_ref_out"]).max(axis=1) > 0)


@pytest.mark.parametrize("branch", list(CASES))
def test_gated_rows_come_back_as_they_went_in(env, branch):
    dt = np.float64
    B, _, members = CASES[branch]
    assert _branch(B, dt, members, True) == branch
    w = _workload(env, B, dt)
    eng = _engine(env, w, dt)
    free = _host_step(env, eng, w, members, active=np.ones(B, dtype=np.int32) if branch == "per_member" else None)
    eng.close()
    eng = _engine(env, w, dt)
    into = {}
    for k in members[1]:
        shape, kdt = eng._out_spec(k)
        into[k] = np.full(shape, -7 if k == "status" else SENTINEL, dtype=kdt)
    before = {k: v.copy() for k, v in into.items()}
    got = _host_step(env, eng, w, members, active=w["gate"], into=into)
    eng.close()
    run = w["gate"] != 0
    assert 0 < run.sum() < B
    for k in members[1]:
        assert got[k] is into[k]
        assert got[k][~run].tobytes() == before[k][~run].tobytes(), "%s: a gated row was written" % k
        assert got[k][run].tobytes() == free[k][run].tobytes(), "%s: a running row differs from the ungated run" % k


@pytest.mark.parametrize("B", [37, 700])
def test_rollout_host_under_the_gate(env, B):
    dt, n_cycles, step = np.float64, 3, 0.01
    w = _workload(env, B, dt)
    eng = _engine(env, w, dt)
    got = eng.rollout_host(w["q"], n_cycles, step, null_control=w["ctrl"], want=("qdot_out", "status"), active=w["gate"])
    with pytest.raises(env.engine.VfikError, match="io->track_error / io->obj_dist are per control cycle: vfik_step only, not a rollout"):
        eng.rollout_host(w["q"], n_cycles, step, null_control=w["ctrl"], want=("qdot_out", "track_error"))
    with pytest.raises(ValueError, match="null_control must be"):
        eng.rollout_host(w["q"], n_cycles, step, null_control=w["ctrl"][:, :3])
    eng.close()
    eng = _engine(env, w, dt)   # the device-pointer rollout under the same gate
    d_q, d_c, d_out, d_qout, d_gate = (eng.dev_alloc(a.nbytes) for a in (w["q"], w["ctrl"], w["q"], w["q"], w["gate"]))
    for p, a in ((d_q, w["q"]), (d_c, w["ctrl"]), (d_gate, w["gate"]), (d_qout, w["q"]), (d_out, np.zeros_like(w["q"]))):
        eng.h2d(p, a)
    eng.rollout(eng.make_io(d_q, null_control=d_c, active=d_gate, qdot_out=d_out), n_cycles, step, q_out=d_qout)
    eng.sync()
    q_dev, qdot_dev = np.zeros_like(w["q"]), np.zeros_like(w["q"])
    eng.d2h(q_dev, d_qout)
    eng.d2h(qdot_dev, d_out)
    for p in (d_q, d_c, d_out, d_qout, d_gate):
        eng.dev_free(p)
    eng.close()
    run = w["gate"] != 0
    assert got["q"][~run].tobytes() == w["q"][~run].tobytes()
    assert got["q"][run].tobytes() == q_dev[run].tobytes() and np.abs(q_dev - w["q"]).max() > 1e-4
    assert got["qdot_out"][run].tobytes() == qdot_dev[run].tobytes() and np.all(got["qdot_out"][~run] == 0.0)


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_submit_host_under_the_gate(env, pinned):
    """Pinned arrays: the direct branch (which of its two forms -- inputs read over the bus, or staged while an earlier submission
    runs -- depends on timing; asserted is what holds in both).  Pageable arrays: the three-stream staging."""
    dt, B, K = np.float64, 300, 3
    w = _workload(env, B, dt)
    rng = np.random.default_rng(9)
    qs = [np.clip(w["q"] + 0.05 * k * rng.normal(size=w["q"].shape), 0.9 * env.chain.q_lo, 0.9 * env.chain.q_hi) for k in range(K)]
    eng = _engine(env, w, dt)
    mk = (lambda shape, d=dt: eng.host_array(shape, d)) if pinned else (lambda shape, d=dt: np.zeros(shape, dtype=d))
    gate, ctrl = mk((B,), np.int32), mk((B, 4))
    gate[:], ctrl[:] = w["gate"], w["ctrl"]
    outs, tickets = [], []
    for k in range(K):   # all submitted before the first wait
        qk = mk((B, 7))
        qk[:] = qs[k]
        o = {"qdot_out": mk((B, 7)), "qdot_null": mk((B, 7)), "pose": mk((B, 16)), "status": mk((B,), np.int32)}
        for name, a in o.items():
            a[:] = -7 if name == "status" else SENTINEL
        outs.append(o)
        tickets.append(eng.submit_host(qk, o, null_control=ctrl, active=gate))
    for t in tickets:
        eng.wait(t)
    outs = [{name: a.copy() for name, a in o.items()} for o in outs]   # (pinned arrays go with their engine)
    eng.close()
    eng = _engine(env, w, dt)
    run = w["gate"] != 0
    for k in range(K):   # (the sign memory of the nullspace advances in submission order, under the same gate)
        ref = eng.step_host(qs[k], null_control=w["ctrl"], want=tuple(outs[k]), active=w["gate"])
        for name, a in outs[k].items():
            assert np.all(a[~run] == (-7 if name == "status" else SENTINEL)), (k, name)
            assert a[run].tobytes() == ref[name][run].tobytes(), (k, name)
    eng.close()


# vfik_device_bytes after each step below, float64 I/O, 64 arms, max_slots 4: read from the library of the commit BEFORE the forms
# shared their staging (this test's sequence run on it on an MI355X; the run's line is in profiles/host_forms_refactor.txt), so that a
# buffer which starts or stops counting shows.  Steps 2 -> 3 and 5 -> 6 grow a stage that exists: its old bytes leave the count.
DEVICE_BYTES = [71808, 84096, 87168, 106880, 106880, 180608]


def test_device_bytes_of_the_grown_buffers(env):
    dt, B = np.float64, 64
    w = _workload(env, B, dt)
    eng = env.engine.Engine(env.chain, B, io_dtype=dt, max_slots=4, params=env.params)
    eng.set_fields(w["fields"], w["nfields"])
    seen = [eng.device_bytes]
    goal = w["fields"]["p"][:, 0, :16].astype(np.float64)
    rep = np.tile(np.array([0.4, 0.1, 0.5, 0.05]), (B, 2, 1))
    eng.move_fields_host(goal=goal, repellers=rep)
    seen.append(eng.device_bytes)
    eng.move_scene_host(goal=goal, repellers=rep, funnels=np.tile(np.array([0.5, 0.0, 0.4, 0.0, 0.0, 1.0]), (B, 1, 1)))
    seen.append(eng.device_bytes)
    eng.goto_host(w["q"], 8, 0.01, (0.01, 0.05), stride=4)
    seen.append(eng.device_bytes)
    eng.goto_host(w["q"], 16, 0.01, (0.01, 0.05))
    seen.append(eng.device_bytes)
    eng.goto_host(w["q"], 16, 0.01, (0.01, 0.05), trajectory=True)   # (the traces: the goto's stage grows)
    seen.append(eng.device_bytes)
    eng.close()
    print("device bytes:", seen)
    assert seen == DEVICE_BYTES
