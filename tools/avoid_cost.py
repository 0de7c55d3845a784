#!/usr/bin/env python
"""What whole-arm avoidance costs (vfik_link_avoid, vfik_set_avoid_rule), measured on one box in one session on C3's batch: 65 536 arms,
7 joints, goal + 8 obstacles, the partner b ^ 1 through a per-arm transform, L = 3 and L = 8 spheres with count = L, float32 and float64
I/O.  Nobody has measured any of this before; no figure is promised, and nothing here is a bar except (d).

 (a) avoid_kernel alone beside clear_kernel and link_kernel alone (they do the same walk) at the same shapes, warm (one handle) and cold
     (handles round-robin, more than the Infinity Cache touched between two uses of one);
 (b) a coupled vfik_goto (nullspace module and mixer, mix_w[4] = 1) under the rule on channel 4 against the same goto on a handle that
     never had a rule (no ext buffer), at strides 4, 10 and 50, per block: avoid_kernel, the memset at the move's end and the ext rows
     the cycles now read;
 (c) tools/resusage.py's lines of avoid_kernel when the build's remarks lie beside the library;
 (d) with --parent-root DIR (a built checkout of the parent commit): the coupled goto without a rule, and bench.py --gpus 1 --steps 200
     --warmup 20, on the parent and on this build, alternating, a process each; this build's medians must lie inside the parent's own
     spread (exit status 1 otherwise).
 --only-kernel: (a) alone.

Every period: HIP events around 200 back-to-back iterations on one stream; per configuration THREE series, alternating over the
configurations, each the median of 9 repetitions after 2 untimed ones.  Into profiles/avoid_cost.txt (--out)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "avoid_cost.txt"))
ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: part (d)")
ap.add_argument("--cold-sets", type=int, default=8)
ap.add_argument("--bench-reps", type=int, default=4)
ap.add_argument("--only-kernel", action="store_true")
ap.add_argument("--coupled-goto-child", action="store_true", help=argparse.SUPPRESS)   # part (d)'s child process: prints one JSON line
args = ap.parse_args()
sys.path.insert(0, os.getcwd() if args.coupled_goto_child else HERE)
import torch  # noqa: E402

from vfclik_amd import _abi, engine, robots, synth  # noqa: E402

chain = robots.lwr()
B, NOBS, K, R, SERIES = 65536, 8, 200, 9, 3
DT, PREC = 0.01, (0.01, 0.05)
L_ALL = (3, 8)
LINKS = (4, 6, 7, 2, 5, 3, 1, 7)
GAIN, D0 = 0.4, 0.2
MIXER = dict(flags=_abi.F_NULLSPACE | _abi.F_MIXER, max_vel=0.7, mix_w=[1.0, 1.0, 0.0, 0.0, 1.0, 0.0])
out_lines = []
failed = False


def say(s=""):
    print(s, flush=True)
    out_lines.append(s)


def period(fn):
    """median over R repetitions (after 2 untimed) of the HIP-event time of fn() in us, and of the host's enqueue time"""
    per, enq = [], []
    for r in range(R + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            per.append(e0.elapsed_time(e1) * 1e3)
            enq.append((t1 - t0) * 1e6)
    return float(np.median(per)), float(np.median(enq))


def series(configs):
    """{name: ([median per series], [enqueue median per series])}: SERIES passes over the configurations in turn"""
    res = {name: ([], []) for name, _ in configs}
    for _ in range(SERIES):
        for name, fn in configs:
            p, e = period(fn)
            res[name][0].append(p)
            res[name][1].append(e)
    return res


def fmt(v, div=1.0):
    return "  ".join("%8.2f" % (x / div) for x in v)


stream = torch.cuda.current_stream().cuda_stream
dev = torch.device("cuda", 0)
rng = np.random.default_rng(3)
src_h = (np.arange(B, dtype=np.int32) ^ 1)
xf_h = np.tile(np.eye(3, 4).reshape(12), (B, 1))
xf_h[:, [3, 7, 11]] = rng.uniform(-0.5, 0.5, size=(B, 3))


def make_set(io, L, seed, params=None, new_calls=True):
    w = synth.make_workload(chain, B, NOBS, seed=seed, io_dtype=io)
    eng = engine.Engine(chain, B, io_dtype=io, max_slots=NOBS, params=params or _abi.default_params(flags=0, max_vel=0.7))
    eng.set_fields(w["fields"], w["nfields"])
    eng.use_stream(stream)
    eng.set_link_spheres([(LINKS[j], (0.01 * j, -0.02, 0.03), 0.05 + 0.004 * j) for j in range(L)])
    tt = getattr(torch, np.dtype(io).name)
    q = torch.from_numpy(w["q"].astype(io)).to(dev)
    qd = torch.zeros(B, 7, dtype=tt, device=dev)
    src = torch.from_numpy(src_h).to(dev)
    xf = torch.from_numpy(xf_h.astype(io)).to(dev)
    rep = torch.zeros(B, L, 4, dtype=tt, device=dev)
    clear = torch.zeros(B, dtype=tt, device=dev)
    pair = torch.zeros(B, dtype=torch.int32, device=dev)
    cmd = torch.zeros(B, 7, dtype=tt, device=dev)
    lib, h = eng.lib, eng.h
    pq, ps, px, pr, pc, pp, pm = (C.c_void_p(t.data_ptr()) for t in (q, src, xf, rep, clear, pair, cmd))

    def link():
        if lib.vfik_link_points(h, pq, ps, px, pr, L, 0):
            raise RuntimeError("vfik_link_points failed")

    def clr():
        if lib.vfik_link_clearance(h, pq, pr, L, 0, L, None, pc, pp):
            raise RuntimeError("vfik_link_clearance failed")

    def avoid():
        if lib.vfik_link_avoid(h, pq, pr, L, 0, L, None, GAIN, D0, None, pm, -1):
            raise RuntimeError("vfik_link_avoid failed")
    link()
    active = None
    if new_calls:
        avoid()
        torch.cuda.synchronize()
        active = float((cmd != 0).any(dim=1).float().mean())
    return dict(eng=eng, link=link, clear=clr, avoid=avoid, active=active, keep=(q, qd, src, xf, rep, clear, pair, cmd, w))


def coupled_set(L, new_calls=True):
    """a float32 set with the mixer under a coupling, and go(stride): one vfik_goto of K cycles on it"""
    s = make_set(np.float32, L, 1, params=_abi.default_params(**MIXER), new_calls=new_calls)
    eng, q = s["eng"], s["keep"][0]
    arrived = torch.zeros(B, dtype=torch.int32, device=dev)
    pending = torch.zeros(K, dtype=torch.int32, device=dev)
    io_c = eng.make_io(q, qdot_out=s["keep"][1])
    eng.set_coupling(src_arm=s["keep"][2], xform=s["keep"][3], first_rep=0)

    def go(stride):
        n = K // stride
        return lambda: eng.goto(io_c, K, DT, PREC, stride=stride, hold=False, clamp=True, arrived=arrived, pending=pending[:n])
    return s, eng, go


if args.coupled_goto_child:
    s, eng, go = coupled_set(3, new_calls=False)   # (nothing of the new entry points: the parent's library runs this too)
    print(json.dumps({"coupled_goto_us": [period(go(10))[0] for _ in range(SERIES)]}), flush=True)
    eng.close()
    sys.exit(0)

say("avoid_cost -- tools/avoid_cost.py; device: %s; ABI %d" % (torch.cuda.get_device_name(0), _abi.ABI_VERSION))
say("times in microseconds; every figure: the medians of %d alternating series of %d repetitions of %d back-to-back iterations" % (SERIES, R, K))
say("batch: %d arms, 7 joints, goal + %d obstacles (C3), the partner b ^ 1 through a transform per arm, spheres on links %s, count = L, gain %.2f, d0 %.2f"
    % (B, NOBS, LINKS, GAIN, D0))
say()

alone = {}
say("(a) avoid_kernel alone, beside clear_kernel and link_kernel (the same walk)")
for io in (np.float32, np.float64):
    esz = np.dtype(io).itemsize
    for L in L_ALL:
        sets = [make_set(io, L, 1 + k) for k in range(args.cold_sets)]
        torch.cuda.synchronize()
        avoid_b = B * 7 * esz + B * L * 4 * esz + B * 7 * esz        # q and L rows in (once); the command out
        say("%s I/O, L = %d: avoid_kernel moves %.2f MB (q, %d rows in; the command out), %.1f KiB of LDS a workgroup; %.0f %% of the arms have an active pair"
            % (np.dtype(io).name, L, avoid_b / 1e6, L, 7 * 3.5 + L * esz / 4, 100 * sets[0]["active"]))
        for state, use in (("warm", sets[:1]), ("cold", sets)):
            def loop(what, use=use):
                def fn():
                    for i in range(K):
                        use[i % len(use)][what]()
                return fn
            res = series([("avoid", loop("avoid")), ("clear", loop("clear")), ("link", loop("link"))])
            for name in ("avoid", "clear", "link"):
                say("    %s [%-5s] per iteration: %s   enqueue: %s" % (state, name, fmt(res[name][0], K), fmt(res[name][1], K)))
            t_avoid, t_clear, t_link = (float(np.median(res[k][0])) / K for k in ("avoid", "clear", "link"))
            alone[np.dtype(io).name, L, state] = t_avoid
            enq = float(np.median(res["avoid"][1])) / K
            say("    %s: avoid_kernel alone %.2f us, clear_kernel alone %.2f us, link_kernel alone %.2f us%s" % (
                state, t_avoid, t_clear, t_link, "  (the host's enqueue, %.2f us, bounds avoid_kernel's period)" % enq if enq > 0.9 * t_avoid else ""))
        for s in sets:
            s["eng"].close()
        del sets
        say()

if not args.only_kernel:
    say("(b) a coupled vfik_goto of %d cycles, float32 I/O, nullspace module + mixer, mix_w[4] = 1, clamp on, no trace, warm: under the rule on channel 4 "
        "against a handle that never had one, per block" % K)
    for L in L_ALL:
        _s0, plain, go_plain = coupled_set(L)
        _s1, ruled, go_ruled = coupled_set(L)
        ruled.set_avoid_rule(GAIN, D0, channel=4)
        for stride in (4, 10, 50):
            n = K // stride
            res = {"no rule": [], "rule": []}
            for _ in range(SERIES):
                res["no rule"].append(period(go_plain(stride))[0])
                res["rule"].append(period(go_ruled(stride))[0])
            u, c = float(np.median(res["no rule"])), float(np.median(res["rule"]))
            spread = (max(res["no rule"]) - min(res["no rule"])) / n
            say("    L = %d, stride %2d (%3d blocks): no rule %s   rule %s" % (L, stride, n, fmt(res["no rule"]), fmt(res["rule"])))
            say("        per block: (%.2f - %.2f) / %d = %.2f us; avoid_kernel alone (warm): %.2f us; the ruleless goto's own spread per block: %.2f us "
                "(the rest: %d cycles a block that read the ext rows, and the memset at the end)" % (c, u, n, (c - u) / n, alone["float32", L, "warm"], spread, stride))
        plain.close()
        ruled.close()
    say()

    say("(c) registers and scratch of avoid_kernel (tools/resusage.py on the build's remarks)")
    r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "resusage.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    rows = [ln for ln in r.stdout.splitlines() if "avoid_kernel" in ln] if r.returncode == 0 else ["tools/resusage.py failed (exit %d)" % r.returncode]
    failed |= r.returncode != 0
    for ln in rows or ["    no remarks beside the library (they are written by the build and are no part of a checkout)"]:
        say("    " + ln.strip())
    say()

    say("(d) rule off, parent and this build alternating, a process each: the coupled goto (L = 3, stride 10; us per goto) and bench.py --gpus 1 --steps 200 --warmup 20 (us per step)")
    if args.parent_root is None:
        say("    not measured (no --parent-root)")
    else:
        me = os.path.abspath(__file__)
        kinds = (("coupled goto", [sys.executable, me, "--coupled-goto-child"], lambda d: float(np.median(d["coupled_goto_us"]))),
                 ("bench.py", [sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], lambda d: d["ms_per_step"] * 1e3))
        for what, cmd, pick in kinds:
            vals = {"parent": [], "this build": []}
            runs = [(label, root) for _ in range(args.bench_reps) for label, root in (("parent", args.parent_root), ("this build", HERE))]
            for label, root in runs:
                p = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                if p.returncode != 0 or not line:   # it may have faulted the GPU: nothing more is started on it
                    say("    %s, %s: FAILED (exit %d); no further run is started" % (what, label, p.returncode))
                    failed = True
                    vals = None
                    break
                vals[label].append(pick(json.loads(line[-1])))
            if vals is None:
                break
            for label, v in vals.items():
                say("    %-12s %-10s median %.3f  min %.3f  max %.3f   runs: %s" % (what, label, np.median(v), min(v), max(v), " ".join("%.3f" % x for x in v)))
            pm, spread = float(np.median(vals["parent"])), max(vals["parent"]) - min(vals["parent"])
            tm = float(np.median(vals["this build"]))
            ok = tm <= pm + spread
            failed |= not ok
            say("    THE BAR, %s: this build's median %.3f is not above the parent's %.3f by more than the parent's own spread %.3f : %s"
                % (what, tm, pm, spread, "PASS" if ok else "MISSED"))

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(out_lines) + "\n")
sys.exit(1 if failed else 0)
