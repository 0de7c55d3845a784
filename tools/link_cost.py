#!/usr/bin/env python
"""What placing the other arm's link spheres costs (vfik_link_points, vfik_set_coupling), measured on one box in one session on C3's batch:
65 536 arms, 7 joints, goal + 8 obstacles, sources b ^ 1 through a per-arm transform, L = 3 and L = 8 spheres, float32 and float64 I/O.
Nobody has measured any of this before; no figure is promised, and nothing here is a bar except (f).

 the floor: one small dependent load -> store launch (tools/ubench_launch, 1024 workgroups of 64 lanes), in the same session;
 (a) link_kernel alone and move_kernel alone (the same L rows), warm (one handle) and cold (handles round-robin, more than the Infinity
     Cache touched between two uses of one); link_kernel against the floor plus its bytes at the rate move_kernel reaches here;
 (b) [link_points; move_fields; step] against [move_fields; step], warm and cold;
 (c) a coupled vfik_goto against the uncoupled one at strides 4, 10 and 50, per block; the expectation is the sum of the two launches
     measured alone in (a), within the uncoupled goto's own spread -- said so, with the figure, where it is missed;
 (d) what a caller has today: one cycle of q read-back -> Chain.fk per link on the host -> move_fields_host, wall clock;
 (e) tools/resusage.py's lines of link_kernel when the build's remarks lie beside the library;
 (f) with --parent-root DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 200 --warmup 20 on the parent and on this
     build, alternating, a process each; this build's median must lie inside the parent's own spread (exit status 1 otherwise).

Every period: HIP events around 200 back-to-back iterations on one stream; per configuration THREE series, alternating over the
configurations, each the median of 9 repetitions after 2 untimed ones.  Into profiles/link_points_cost.txt (--out)."""
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
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "link_points_cost.txt"))
ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: part (f)")
ap.add_argument("--cold-sets", type=int, default=8)
ap.add_argument("--bench-reps", type=int, default=4)
args = ap.parse_args()
sys.path.insert(0, HERE)
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


say("link_points_cost -- tools/link_cost.py; device: %s; ABI %d" % (torch.cuda.get_device_name(0), _abi.ABI_VERSION))
say("times in microseconds; every figure: the medians of %d alternating series of %d repetitions of %d back-to-back iterations" % (SERIES, R, K))
say("batch: %d arms, 7 joints, goal + %d obstacles (C3), sources b ^ 1, a transform per arm, spheres on links %s" % (B, NOBS, LINKS))
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

stream = torch.cuda.current_stream().cuda_stream
dev = torch.device("cuda", 0)
rng = np.random.default_rng(3)
src_h = (np.arange(B, dtype=np.int32) ^ 1)
xf_h = np.tile(np.eye(3, 4).reshape(12), (B, 1))
xf_h[:, [3, 7, 11]] = rng.uniform(-0.5, 0.5, size=(B, 3))
alone = {}


def make_set(io, L, seed, flags=0):
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
    step = eng.stepper(eng.make_io(q, qdot_out=qd))
    lib, h = eng.lib, eng.h
    pq, ps, px, pr = (C.c_void_p(t.data_ptr()) for t in (q, src, xf, rep))

    def link():
        if lib.vfik_link_points(h, pq, ps, px, pr, L, 0):
            raise RuntimeError("vfik_link_points failed")

    def move():
        if lib.vfik_move_fields(h, 0, B, None, pr, L, None):
            raise RuntimeError("vfik_move_fields failed")
    link()
    return dict(eng=eng, link=link, move=move, step=step, keep=(q, qd, src, xf, rep, w))


for io in (np.float32, np.float64):
    esz = np.dtype(io).itemsize
    for L in L_ALL:
        sets = [make_set(io, L, 1 + k) for k in range(args.cold_sets)]
        torch.cuda.synchronize()
        link_b = B * 7 * esz + B * 4 + B * 12 * esz + B * L * 4 * esz                  # q, src_arm, xform in; L rows out
        move_b = B * L * 4 * esz + B * NOBS * 2 + B * L * (4 + 4 + 4) * esz            # rows and slot map in; uniform, compact and general image out
        say("%s I/O, L = %d: link_kernel moves %.2f MB (q, src_arm, xform12 in; %d rows out), move_kernel %.2f MB" % (np.dtype(io).name, L, link_b / 1e6, L, move_b / 1e6))
        for state, use in (("warm", sets[:1]), ("cold", sets)):
            def loop(what, use=use):
                def fn():
                    for i in range(K):
                        s = use[i % len(use)]
                        for w_ in what:
                            s[w_]()
                return fn
            res = series([("link", loop(("link",))), ("move", loop(("move",))), ("move+step", loop(("move", "step"))),
                          ("link+move+step", loop(("link", "move", "step")))])
            for name in ("link", "move", "move+step", "link+move+step"):
                say("    %s (a/b) [%-14s] per iteration: %s   enqueue: %s" % (state, name, fmt(res[name][0], K), fmt(res[name][1], K)))
            t_link, t_move = float(np.median(res["link"][0])) / K, float(np.median(res["move"][0])) / K
            rate = move_b / t_move / 1e6
            alone[np.dtype(io).name, L, state] = (t_link, t_move)
            enq_l = float(np.median(res["link"][1])) / K
            say("    %s: move_kernel alone %.2f us = %.2f TB/s; link_kernel alone %.2f us%s" % (
                state, t_move, rate, t_link, "  (the host's enqueue, %.2f us, bounds this period)" % enq_l if enq_l > 0.9 * t_link else ""))
            if floor is not None:
                say("    %s: link_kernel against the floor plus its bytes at that rate: %.2f us  vs  %.2f + %.2f = %.2f us" % (
                    state, t_link, floor, link_b / rate / 1e6, floor + link_b / rate / 1e6))
            d = float(np.median(res["link+move+step"][0])) / K - float(np.median(res["move+step"][0])) / K
            say("    %s: [link_points; move_fields; step] - [move_fields; step] = %.2f us per cycle" % (state, d))
        for s in sets:
            s["eng"].close()
        del sets
        say()

say("(c) vfik_goto of %d cycles, float32 I/O, flags 0, clamp on, no trace, warm: coupled against uncoupled, per block" % K)
for L in L_ALL:
    s = make_set(np.float32, L, 1)
    eng = s["eng"]
    q = s["keep"][0]
    arrived = torch.zeros(B, dtype=torch.int32, device=dev)
    pending = torch.zeros(K, dtype=torch.int32, device=dev)
    io_c = eng.make_io(q, qdot_out=s["keep"][1])
    for stride in (4, 10, 50):
        n = K // stride

        def go(n=n, stride=stride):
            eng.goto(io_c, K, DT, PREC, stride=stride, hold=False, clamp=True, arrived=arrived, pending=pending[:n])

        def couple(on):
            def fn():
                if on:
                    eng.set_coupling(src_arm=s["keep"][2], xform=s["keep"][3], first_rep=0)
                else:
                    eng.set_coupling(None)
            return fn
        res = {"uncoupled": [], "coupled": []}
        for _ in range(SERIES):
            for name in ("uncoupled", "coupled"):
                couple(name == "coupled")()
                res[name].append(period(go)[0])
        eng.set_coupling(None)
        u, c = float(np.median(res["uncoupled"])), float(np.median(res["coupled"]))
        spread = (max(res["uncoupled"]) - min(res["uncoupled"])) / n
        t_link, t_move = alone["float32", L, "warm"]
        per_block = (c - u) / n
        verdict = "within" if abs(per_block - (t_link + t_move)) <= spread else "NOT within"
        say("    L = %d, stride %2d (%3d blocks): uncoupled %s   coupled %s" % (L, stride, n, fmt(res["uncoupled"]), fmt(res["coupled"])))
        say("        per block: (%.2f - %.2f) / %d = %.2f us; the two launches alone: %.2f + %.2f = %.2f us; the uncoupled goto's own spread per block: %.2f us: %s it"
            % (c, u, n, per_block, t_link, t_move, t_link + t_move, spread, verdict))
    eng.close()
say()

say("(d) what a caller has today, one cycle: q read-back -> Chain.fk per link on the host -> move_fields_host; wall clock, float32 I/O")
for L in L_ALL:
    s = make_set(np.float32, L, 1)
    eng, q = s["eng"], s["keep"][0]
    spheres = [(LINKS[j], (0.01 * j, -0.02, 0.03), 0.05 + 0.004 * j) for j in range(L)]
    ts = []
    for r in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        qh = q.cpu().numpy().astype(np.float64)
        rows = np.zeros((B, L, 4))
        qs = qh[src_h]
        fk = {}
        for j, (link, c, rad) in enumerate(spheres):
            if link not in fk:
                sub = type(chain)(chain.B[: link + 1], chain.jtype[:link], chain.q_lo[:link], chain.q_hi[:link])
                fk[link] = sub.fk(qs[:, :link])
            P = fk[link][:, :3, :3] @ np.asarray(c) + fk[link][:, :3, 3]
            rows[:, j, :3] = P + xf_h[:, [3, 7, 11]]
            rows[:, j, 3] = rad
        eng.move_fields_host(repellers=rows)
        ts.append((time.perf_counter() - t0) * 1e6)
    say("    L = %d: %s us per cycle (5 runs, the first included: %s)" % (L, "%.0f" % np.median(ts[1:]), " ".join("%.0f" % t for t in ts)))
    eng.close()
say()

say("(e) registers and scratch of link_kernel (tools/resusage.py on the build's remarks)")
r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "resusage.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
rows = [ln for ln in r.stdout.splitlines() if "link_kernel" in ln] if r.returncode == 0 else ["tools/resusage.py failed (exit %d)" % r.returncode]
failed |= r.returncode != 0
for ln in rows or ["    no remarks beside the library (they are written by the build and are no part of a checkout)"]:
    say("    " + ln.strip())
say()

say("(f) bench.py --gpus 1 --steps 200 --warmup 20, parent and this build alternating, a process each: us per step")
if args.parent_root is None:
    say("    not measured (no --parent-root)")
else:
    vals = {"parent": [], "this build": []}
    runs = [(label, root) for _ in range(args.bench_reps) for label, root in (("parent", args.parent_root), ("this build", HERE))]
    for label, root in runs:
        p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=root, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:   # it may have faulted the GPU: nothing more is started on it
            say("    %s: FAILED (exit %d); no further run is started" % (label, p.returncode))
            failed = True
            vals = {"parent": [], "this build": []}
            break
        vals[label].append(json.loads(line[-1])["ms_per_step"] * 1e3)
    for label, v in vals.items():
        if v:
            say("    %-10s median %.3f  min %.3f  max %.3f   runs: %s" % (label, np.median(v), min(v), max(v), " ".join("%.3f" % x for x in v)))
    if vals["parent"] and vals["this build"]:
        pm, spread = float(np.median(vals["parent"])), max(vals["parent"]) - min(vals["parent"])
        tm = float(np.median(vals["this build"]))
        ok = tm <= pm + spread
        failed |= not ok
        say("    THE BAR: this build's median %.3f is not above the parent's %.3f by more than the parent's own spread %.3f : %s" % (tm, pm, spread, "PASS" if ok else "MISSED"))

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(out_lines) + "\n")
sys.exit(1 if failed else 0)
