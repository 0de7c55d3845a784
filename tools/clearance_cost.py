#!/usr/bin/env python
"""What measuring link-sphere clearance costs (vfik_link_clearance, vfik_set_wait_rule), measured on one box in one session on C3's batch:
65 536 arms, 7 joints, goal + 8 obstacles, the partner b ^ 1 through a per-arm transform, L = 3 and L = 8 spheres with count = L, float32
and float64 I/O.  Nobody has measured any of this before; no figure is promised, and nothing here is a bar except (d).

 the floor: one small dependent load -> store launch (tools/ubench_launch, 1024 workgroups of 64 lanes), in the same session;
 (a) clear_kernel alone beside link_kernel alone (it does the same walk) and move_kernel alone (the rate this session reaches), warm (one
     handle) and cold (handles round-robin, more than the Infinity Cache touched between two uses of one); clear_kernel against the floor
     plus its bytes at move_kernel's rate;
 (b) a coupled vfik_goto under a wait rule nobody meets (the measurement runs, nobody waits: the same cycles) against the coupled goto
     without a rule at strides 4, 10 and 50, per block; the expectation is clear_kernel alone from (a) plus what running under the gate
     costs, said with the figure;
 (c) tools/resusage.py's lines of clear_kernel when the build's remarks lie beside the library;
 (d) with --parent-root DIR (a built checkout of the parent commit): the coupled goto without a rule, and bench.py --gpus 1 --steps 200
     --warmup 20, on the parent and on this build, alternating, a process each; this build's medians must lie inside the parent's own
     spread (exit status 1 otherwise).
 --only-kernel: (a) alone (what an A/B of two builds of the kernel runs).

Every period: HIP events around 200 back-to-back iterations on one stream; per configuration THREE series, alternating over the
configurations, each the median of 9 repetitions after 2 untimed ones.  Into profiles/clearance_cost.txt (--out)."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "clearance_cost.txt"))
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


def make_set(io, L, seed, flags=0, clearance=True):
    w = synth.make_workload(chain, B, NOBS, seed=seed, io_dtype=io)
    eng = engine.Engine(chain, B, io_dtype=io, max_slots=NOBS, params=_abi.default_params(flags=flags, max_vel=0.7))
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
    lib, h = eng.lib, eng.h
    pq, ps, px, pr, pc, pp = (C.c_void_p(t.data_ptr()) for t in (q, src, xf, rep, clear, pair))

    def link():
        if lib.vfik_link_points(h, pq, ps, px, pr, L, 0):
            raise RuntimeError("vfik_link_points failed")

    def move():
        if lib.vfik_move_fields(h, 0, B, None, pr, L, None):
            raise RuntimeError("vfik_move_fields failed")

    def clr():
        if lib.vfik_link_clearance(h, pq, pr, L, 0, L, None, pc, pp):
            raise RuntimeError("vfik_link_clearance failed")
    link()
    if clearance:
        clr()
    return dict(eng=eng, link=link, move=move, clear=clr, keep=(q, qd, src, xf, rep, clear, pair, w))


def coupled_set(L, clearance=True):
    """a float32 set under a coupling, and go(stride): one vfik_goto of K cycles on it"""
    s = make_set(np.float32, L, 1, clearance=clearance)
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
    s, eng, go = coupled_set(3, clearance=False)   # (nothing of the new entry points: the parent's library runs this too)
    print(json.dumps({"coupled_goto_us": [period(go(10))[0] for _ in range(SERIES)]}), flush=True)
    eng.close()
    sys.exit(0)

say("clearance_cost -- tools/clearance_cost.py; device: %s; ABI %d" % (torch.cuda.get_device_name(0), _abi.ABI_VERSION))
say("times in microseconds; every figure: the medians of %d alternating series of %d repetitions of %d back-to-back iterations" % (SERIES, R, K))
say("batch: %d arms, 7 joints, goal + %d obstacles (C3), the partner b ^ 1 through a transform per arm, spheres on links %s, count = L" % (B, NOBS, LINKS))
say()

floor = None
ub = os.path.join(HERE, "tools", "ubench_launch")
if os.path.exists(ub):
    r = subprocess.run([ub], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    if r.returncode != 0:   # a program that failed on the GPU: nothing more is started on it
        sys.exit("tools/ubench_launch failed (exit %d): %s" % (r.returncode, r.stderr.strip()[-300:]))
    for ln in r.stdout.splitlines():
        m = re.match(r"\s*1024\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)", ln)
        if m:
            floor = float(m.group(2))
            say("the floor (tools/ubench_launch, 1024 workgroups of 64 lanes, back-to-back period): empty %.2f, load+store %.2f, const+load+store %.2f us"
                % (float(m.group(1)), floor, float(m.group(3))))
if floor is None:
    say("the floor: tools/ubench_launch is not built (make -C tools ubench_launch): NOT measured")
say()

alone = {}
say("(a) clear_kernel alone, beside link_kernel (the same walk) and move_kernel (this session's rate)")
for io in (np.float32, np.float64):
    esz = np.dtype(io).itemsize
    for L in L_ALL:
        sets = [make_set(io, L, 1 + k) for k in range(args.cold_sets)]
        torch.cuda.synchronize()
        link_b = B * 7 * esz + B * 4 + B * 12 * esz + B * L * 4 * esz                  # q, src_arm, xform in; L rows out
        move_b = B * L * 4 * esz + B * NOBS * 2 + B * L * (4 + 4 + 4) * esz            # rows and slot map in; uniform, compact and general image out
        clear_b = B * 7 * esz + B * L * 4 * esz + B * esz + B * 4                      # q and L rows in (once); clear and pair out
        say("%s I/O, L = %d: clear_kernel moves %.2f MB when every row is read from memory once (q, %d rows in; clear, pair out) and asks for its rows %d times; "
            "link_kernel %.2f MB, move_kernel %.2f MB" % (np.dtype(io).name, L, clear_b / 1e6, L, L, link_b / 1e6, move_b / 1e6))
        for state, use in (("warm", sets[:1]), ("cold", sets)):
            def loop(what, use=use):
                def fn():
                    for i in range(K):
                        use[i % len(use)][what]()
                return fn
            res = series([("clear", loop("clear")), ("link", loop("link")), ("move", loop("move"))])
            for name in ("clear", "link", "move"):
                say("    %s [%-5s] per iteration: %s   enqueue: %s" % (state, name, fmt(res[name][0], K), fmt(res[name][1], K)))
            t_clear, t_link, t_move = (float(np.median(res[k][0])) / K for k in ("clear", "link", "move"))
            rate = move_b / t_move / 1e6
            alone[np.dtype(io).name, L, state] = t_clear
            enq = float(np.median(res["clear"][1])) / K
            say("    %s: clear_kernel alone %.2f us, link_kernel alone %.2f us, move_kernel alone %.2f us = %.2f TB/s%s" % (
                state, t_clear, t_link, t_move, rate, "  (the host's enqueue, %.2f us, bounds clear_kernel's period)" % enq if enq > 0.9 * t_clear else ""))
            if floor is not None:
                say("    %s: clear_kernel against the floor plus its bytes at that rate: %.2f us  vs  %.2f + %.2f = %.2f us" % (
                    state, t_clear, floor, clear_b / rate / 1e6, floor + clear_b / rate / 1e6))
        for s in sets:
            s["eng"].close()
        del sets
        say()

if not args.only_kernel:
    say("(b) a coupled vfik_goto of %d cycles, float32 I/O, flags 0, clamp on, no trace, warm: under a wait rule nobody meets against no rule, per block" % K)
    for L in L_ALL:
        s, eng, go = coupled_set(L)
        for stride in (4, 10, 50):
            n = K // stride
            res = {"no rule": [], "rule": []}
            for _ in range(SERIES):
                for name in ("no rule", "rule"):
                    eng.set_wait_rule(-1e30 if name == "rule" else None)   # (strict compare: no clearance is below it)
                    res[name].append(period(go(stride))[0])
            eng.set_wait_rule(None)
            u, c = float(np.median(res["no rule"])), float(np.median(res["rule"]))
            spread = (max(res["no rule"]) - min(res["no rule"])) / n
            per_block = (c - u) / n
            say("    L = %d, stride %2d (%3d blocks): no rule %s   rule %s" % (L, stride, n, fmt(res["no rule"]), fmt(res["rule"])))
            say("        per block: (%.2f - %.2f) / %d = %.2f us; clear_kernel alone (warm): %.2f us; the ruleless goto's own spread per block: %.2f us "
                "(the rest: the cycles run under the handle's gate)" % (c, u, n, per_block, alone["float32", L, "warm"], spread))
        eng.close()
    say()

    say("(c) registers and scratch of clear_kernel (tools/resusage.py on the build's remarks)")
    r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "resusage.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    rows = [ln for ln in r.stdout.splitlines() if "clear_kernel" in ln] if r.returncode == 0 else ["tools/resusage.py failed (exit %d)" % r.returncode]
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
