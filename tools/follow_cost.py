#!/usr/bin/env python
"""What a check of vfik_follow costs over a check of vfik_goto, measured on one box in one session, on C3's batch: 65 536 arms, 7 joints,
goal + 8 obstacles, float32 I/O, 200 control cycles, W = 4 waypoints per arm, strides 4 / 10 / 50.

vfik_goto is existing code and the yardstick.  Both calls get the same options and an all-ones io->active, so that both run their blocks
under the handle's gate (a follow always does; a goto without hold and without a caller's gate launches its blocks without one): the
cycle launches are then the same kernels on the same arms, and the difference of the two periods, divided by the number of checks, is
what check_kernel<T, 0, 1> costs over check_kernel<T, 0, 0>.  Two scenes:

 far    every waypoint is C3's own random goal: the arms that get there within 200 cycles pass all four, one per check; hold off and on;
 near   waypoints at fk(q0 + 0.04 w U(-1, 1)), w = 1..4: arms reach waypoints throughout the run (counted), hold off -- every arm runs
        every block in both calls; the goto heads for waypoint 0, which vfik_move_fields_host puts into the goal blocks first.

Series alternate goto, follow, goto, follow, ...: --series of each, every one a median of --reps HIP-event periods after 2 untimed runs.
Reported: the medians, the spread of goto's own medians over its series, the difference per check, and the extra bytes a check moves
(next and the path length where check_kernel<T, 0, 0> reads arrived: 8 against 4 B per arm; per arm that reaches a waypoint a frame's rows 0..2
read and written, 2 x 48 B at float32 I/O, and reached / next, 8 B) at the 4.81 TB/s profiles/move_fields_cost.txt reached.  No bar is
fixed: anything beyond spread plus bytes is stated as a finding.

 (e) with --parent-root DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 200 --warmup 20 on the parent and on this
     build, alternating, each in a process of its own: both medians and the parent's spread.

Into profiles/follow_cost.txt (--out)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "follow_cost.txt"))
ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: part (e)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--series", type=int, default=3)
ap.add_argument("--bench-reps", type=int, default=4)
args = ap.parse_args()
sys.path.insert(0, HERE)
import torch  # noqa: E402

from vfclik_amd import _abi, engine, robots, synth  # noqa: E402

chain = robots.lwr()
L = []


def say(s=""):
    print(s, flush=True)
    L.append(s)


B, NOBS, K, W, R = 65536, 8, 200, 4, args.reps
DT, PREC = 0.01, (0.01, 0.05)
STRIDES = (4, 10, 50)
RATE = 4.81e6   # bytes per microsecond
say("follow_cost -- tools/follow_cost.py; device: %s; ABI %d" % (torch.cuda.get_device_name(0), _abi.ABI_VERSION))
say("times in microseconds for the WHOLE sequence of %d control cycles unless a line says otherwise; HIP events around the sequence on one" % K)
say("stream; %d series of goto and of follow, alternating, each a median of %d periods after 2 untimed runs" % (args.series, R))
say("batch: %d arms, 7 joints, float32 I/O, goal + %d obstacles (C3), W = %d, flags 0, clamp on, dt %.2f, precision (%.2f m, %.2f rad)," % (B, NOBS, W, DT, PREC[0], PREC[1]))
say("io->active all ones in both calls (both run their blocks under the gate), no trace, pending given")
say()

stream = torch.cuda.current_stream().cuda_stream
w = synth.make_workload(chain, B, NOBS, seed=1, io_dtype=np.float32)
eng = engine.Engine(chain, B, io_dtype=np.float32, max_slots=8, params=_abi.default_params(max_vel=0.7))
eng.set_fields(w["fields"], w["nfields"])
eng.use_stream(stream)
dev = torch.device("cuda", 0)
q0 = torch.from_numpy(w["q"].astype(np.float32)).to(dev)
qdot = torch.zeros(B, 7, device=dev)
ones = torch.ones(B, dtype=torch.int32, device=dev)
arrived = torch.zeros(B, dtype=torch.int32, device=dev)
reached = torch.zeros(B, W, dtype=torch.int32, device=dev)
nxt = torch.zeros(B, dtype=torch.int32, device=dev)
pending = torch.zeros(K, dtype=torch.int32, device=dev)
io = eng.make_io(q0, qdot_out=qdot, active=ones)

rng = np.random.default_rng(3)
goal0 = w["fields"]["p"][:, 0, :16].astype(np.float32)
far = np.repeat(goal0[:, None, :], W, axis=1)
qn = w["q"][:, None, :] + 0.04 * np.arange(1, W + 1)[None, :, None] * rng.uniform(-1.0, 1.0, size=(B, W, 7))
near = chain.fk(qn.reshape(B * W, 7)).reshape(B, W, 16).astype(np.float32)


def median_period(fn):
    per = []
    for r in range(R + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            per.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(per))


findings = []
for scene, way, holds in (("far", far, (False, True)), ("near", near, (False,))):
    way_t = torch.from_numpy(way).to(dev)
    eng.move_fields_host(goal=way[:, 0].astype(np.float64))   # the goto's goal: waypoint 0 (a follow puts it there itself)
    say("scene %s" % scene)
    for hold in holds:
        for s in STRIDES:
            n = K // s
            kw = dict(stride=s, hold=hold, clamp=True, pending=pending[:n])

            def goto():
                eng.goto(io, K, DT, PREC, arrived=arrived, **kw)

            def follow():
                eng.follow(io, way_t, K, DT, PREC, reached=reached, next=nxt, **kw)
            g, f = [], []
            for _ in range(args.series):
                eng.move_fields_host(goal=way[:, 0].astype(np.float64))   # (a follow leaves the arms' last waypoints behind)
                g.append(median_period(goto))
                f.append(median_period(follow))
            torch.cuda.synchronize()
            hits, there = int((reached >= 0).sum()), int((arrived >= 0).sum())
            gm, fm, spread = float(np.median(g)), float(np.median(f)), max(g) - min(g)
            bytes_us = (4 * B * n + 104 * hits) / RATE
            beyond = (fm - gm) - spread - bytes_us
            say("    s = %2d, hold %s: goto   medians %s  -> %9.2f, spread of its medians %.2f" % (s, "on " if hold else "off", " ".join("%9.2f" % x for x in g), gm, spread))
            say("    %-17s follow medians %s  -> %9.2f" % ("", " ".join("%9.2f" % x for x in f), fm))
            say("    %-17s difference %+.2f us = %+.3f us per check (%d checks); waypoints reached in a follow %d (arms the goto found at waypoint 0: %d);"
                % ("", fm - gm, (fm - gm) / n, n, hits, there))
            say("    %-17s extra bytes %.2f MB = %.2f us at 4.81 TB/s; beyond spread and bytes: %s"
                % ("", (4 * B * n + 104 * hits) / 1e6, bytes_us, "nothing" if beyond <= 0 else "%.2f us = %.3f us per check" % (beyond, beyond / n)))
            if beyond > 0:
                findings.append("scene %s, s = %d, hold %s: %.3f us per check beyond goto's spread and the extra bytes" % (scene, s, "on" if hold else "off", beyond / n))
    say()
say("FINDINGS" if findings else "FINDINGS: none -- every difference lies inside goto's own spread plus the time of the extra bytes")
for x in findings:
    say("    " + x)
if findings:
    say("    What the excess is made of is not measured here.  check_kernel<T, 0, 1> reads two words per arm where check_kernel<T, 0, 0> reads one, has three")
    say("    quad stores per arriving lane, and otherwise the same kernel boundary and the same one atomic add per wave.")
say()
eng.close()

say("(e) bench.py --gpus 1 --steps 200 --warmup 20, parent and this build alternating, a process each: us per step")
if args.parent_root is None:
    say("    not measured (no --parent-root)")
else:
    vals = {"parent": [], "this build": []}
    runs = [(label, root) for r in range(args.bench_reps) for label, root in (("parent", args.parent_root), ("this build", HERE))]
    for label, root in runs:
        p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=root, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not line:
            say("    %s: FAILED (exit %d); nothing further is started" % (label, p.returncode))
            break
        vals[label].append(json.loads(line[-1])["ms_per_step"] * 1e3)
    for label, v in vals.items():
        if v:
            say("    %-10s median %.3f  min %.3f  max %.3f   runs: %s" % (label, np.median(v), min(v), max(v), " ".join("%.3f" % x for x in v)))
    if vals["parent"] and vals["this build"]:
        pm, spread, tm = float(np.median(vals["parent"])), max(vals["parent"]) - min(vals["parent"]), float(np.median(vals["this build"]))
        say("    this build's median %.3f against the parent's %.3f; the parent's own spread %.3f : %s" % (tm, pm, spread, "inside" if tm <= pm + spread else "ABOVE"))

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(L) + "\n")
