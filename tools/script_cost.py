#!/usr/bin/env python
"""What a check of vfik_script costs over the matching check of vfik_follow and of vfik_follow_js, measured on one box in one session, on
C3's batch: 65 536 arms, 7 joints, goal + 8 obstacles, float32 I/O, 200 control cycles, W = 4 steps per arm, strides 4 / 10 / 50.

Two comparisons, in each of which both calls run the same cycle kernels on the same arms with the same numbers, so that as many arms
are under way and advance in both and the difference of the two periods, divided by the number of checks, is what script_kernel<T> costs
over the list check it restates:

 frames    a script of frames only against vfik_follow.  The handle has F_MIXER, mixer [1, 1, 0, 0, 0, 0] and per-arm mixer rows that differ
           in weight 5 alone (a channel nobody feeds), and the follow gets an io->q_ref whose rows start with NaN (no controller): its
           blocks then take the kernel a script's blocks take -- per-arm mixer planes and a reference row.
 postures  a script of postures only against vfik_follow_js, the handle's mixer [0, 0, 1, 0, 0, 0], jp_kp 8, the same per-arm rows.

Waypoints near the start -- fk(q0 + 0.04 w U(-1, 1)) and q0 + 0.04 w U(-1, 1), w = 1..4 --, so that arms advance throughout the run
(counted); hold off, io->active all ones, no trace, pending given.  The kernels each call launched are listed (vfik_launched_kernels).

The calls are made at the C ABI (vfik_follow, vfik_follow_js, vfik_script) on options built beforehand: a period then holds what the
library and the device do and no Python preparation.  (Timed through Engine.follow / Engine.script the difference did not grow with the
number of checks -- 30 / 22 / 12 us per run at 50 / 20 / 4 checks for frames, 43 / 45 / 31 for postures: Engine.script checks more
arrays before its first enqueue, and the device waits for it inside the period.)

Series alternate follow, script, follow, script, ...: --series of each, every one a median of --reps HIP-event periods after 2 untimed
runs.  Reported: the medians, the spread of the follow's own medians over its series, the difference per check, and the extra bytes a
script's check moves (kind: 4 B per arm; the mixer quad: 16 B per arm that advances) at the 4.81 TB/s profiles/move_fields_cost.txt
reached.  Expectation: the difference is no more than that spread plus the time of those bytes; anything beyond is stated as a finding.

 --follow-only   measure the two follow calls alone and print one JSON line: run with --root DIR on a built checkout of the parent commit
                 (--parent-root does that in a process of its own), it gives the follow figures of the parent build in the same session.
 (e) with --parent-root: bench.py --gpus 1 --steps 200 --warmup 20 on the parent and on this build, alternating, a process each.
 (f) with --isa-diff FILE: the summary tools/isa_diff.py wrote for parent against this build, copied in.

Into profiles/script_cost.txt (--out)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "script_cost.txt"))
ap.add_argument("--root", default=HERE, help="the built checkout whose package is measured")
ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its follow figures, and part (e)")
ap.add_argument("--follow-only", action="store_true")
ap.add_argument("--isa-diff", default=None)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--series", type=int, default=3)
ap.add_argument("--bench-reps", type=int, default=4)
args = ap.parse_args()
args.root = os.path.abspath(args.root)
args.parent_root = None if args.parent_root is None else os.path.abspath(args.parent_root)
sys.path.insert(0, args.root)
import torch  # noqa: E402

from vfclik_amd import _abi, engine, robots, synth  # noqa: E402

chain = robots.lwr()
L = []


def say(s=""):
    print(s, file=sys.stderr if args.follow_only else sys.stdout, flush=True)
    L.append(s)


B, NOBS, K, W, R = 65536, 8, 200, 4, args.reps
DT, PREC, KP = 0.01, (0.01, 0.05), 8.0
JS_PREC = 0.004 + 0.002 * np.arange(7)
STRIDES = (4, 10, 50)
RATE = 4.81e6   # bytes per microsecond
say("script_cost -- tools/script_cost.py; device: %s; ABI %d" % (torch.cuda.get_device_name(0), _abi.ABI_VERSION))
say("times in microseconds for the WHOLE sequence of %d control cycles unless a line says otherwise; HIP events around the sequence on one" % K)
say("stream; %d series of the follow and of the script, alternating, each a median of %d periods after 2 untimed runs" % (args.series, R))
say("batch: %d arms, 7 joints, float32 I/O, goal + %d obstacles (C3), W = %d, F_MIXER, clamp on, dt %.2f, precision (%.2f m, %.2f rad) and" % (B, NOBS, W, DT, PREC[0], PREC[1]))
say("0.004 + 0.002 i rad at every step, hold off, io->active all ones, no trace, pending given")
say()

stream = torch.cuda.current_stream().cuda_stream
w = synth.make_workload(chain, B, NOBS, seed=1, io_dtype=np.float32)
dev = torch.device("cuda", 0)
q0 = torch.from_numpy(w["q"].astype(np.float32)).to(dev)
qdot = torch.zeros(B, 7, device=dev)
ones = torch.ones(B, dtype=torch.int32, device=dev)
reached = torch.zeros(B, W, dtype=torch.int32, device=dev)
nxt = torch.zeros(B, dtype=torch.int32, device=dev)
pending = torch.zeros(K, dtype=torch.int32, device=dev)
no_ctl = torch.full((B, 7), float("nan"), device=dev)

rng = np.random.default_rng(3)
qn = w["q"][:, None, :] + 0.04 * np.arange(1, W + 1)[None, :, None] * rng.uniform(-1.0, 1.0, size=(B, W, 7))
way = chain.fk(qn.reshape(B * W, 7)).reshape(B, W, 16).astype(np.float32)
way_t = torch.from_numpy(way).to(dev)
wayq_t = torch.from_numpy(qn.astype(np.float32)).to(dev)
rows = np.tile([0.0] * 6, (B, 1))
rows[1::2, 5] = 1e-3


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


findings, of_follow = [], {}
for form, mix in (("frames", [1.0, 1.0, 0.0, 0.0]), ("postures", [0.0, 0.0, 1.0, 0.0])):
    eng = engine.Engine(chain, B, io_dtype=np.float32, max_slots=8,
                        params=_abi.default_params(flags=_abi.F_MIXER, max_vel=0.7, jp_kp=KP, mix_w=mix + [0.0, 0.0]))
    eng.set_fields(w["fields"], w["nfields"])
    rows[:, :4] = mix
    eng.set_mixer_weights(rows)
    eng.use_stream(stream)
    io_ref = eng.make_io(q0, qdot_out=qdot, active=ones, q_ref=no_ctl)
    io = eng.make_io(q0, qdot_out=qdot, active=ones)
    if not args.follow_only:
        kind_t = torch.full((B, W), _abi.STEP_FRAME if form == "frames" else _abi.STEP_POSTURE, dtype=torch.int32, device=dev)
    say("%s: a script of %s only against %s" % (form, form, "vfik_follow" if form == "frames" else "vfik_follow_js"))
    for s in STRIDES:
        n = K // s

        def options(cls):
            o = eng._move_opts(cls, K, DT, s, False, True)
            o.n_way, o.reached, o.next, o.pending = W, reached.data_ptr(), nxt.data_ptr(), pending.data_ptr()
            return o
        if form == "frames":
            of = options(_abi.FollowOpts)
            eng._follow_precision(of, PREC, None)
            of.way16 = way_t.data_ptr()
            f_fn, f_io = eng.lib.vfik_follow, io_ref
        else:
            of = options(_abi.FollowJsOpts)
            kept_f = eng._follow_js_precision(of, JS_PREC, None)
            of.wayq = wayq_t.data_ptr()
            f_fn, f_io = eng.lib.vfik_follow_js, io
        if not args.follow_only:
            os_, kept_s = eng._script_opts(K, DT, s, False, True, PREC, None, JS_PREC, None, _abi.MIX_FRAME, _abi.MIX_POSTURE)
            os_.n_way, os_.reached, os_.next, os_.pending = W, reached.data_ptr(), nxt.data_ptr(), pending.data_ptr()
            os_.kind, os_.way16, os_.wayq = kind_t.data_ptr(), way_t.data_ptr(), wayq_t.data_ptr()

        def follow():
            eng._chk(f_fn(eng.h, C.byref(f_io), C.byref(of)))

        def script():
            eng._chk(eng.lib.vfik_script(eng.h, C.byref(io), C.byref(os_)))
        f, c, names = [], [], {}
        for _ in range(args.series):
            eng.launched_kernels()
            f.append(median_period(follow))
            names["follow"] = eng.launched_kernels()
            torch.cuda.synchronize()
            hits_f = int((reached >= 0).sum())
            if not args.follow_only:
                c.append(median_period(script))
                names["script"] = eng.launched_kernels()
                torch.cuda.synchronize()
                hits = int((reached >= 0).sum())
        fm, spread = float(np.median(f)), max(f) - min(f)
        of_follow["%s %d" % (form, s)] = f
        say("    s = %2d: follow medians %s  -> %9.2f, spread of its medians %.2f; steps reached %d" % (s, " ".join("%9.2f" % x for x in f), fm, spread, hits_f))
        if args.follow_only:
            continue
        cm = float(np.median(c))
        bytes_us = (4 * B * n + 16 * hits) / RATE
        beyond = (cm - fm) - spread - bytes_us
        say("    %-7s script medians %s  -> %9.2f; steps reached %d" % ("", " ".join("%9.2f" % x for x in c), cm, hits))
        say("    %-7s difference %+.2f us = %+.3f us per check (%d checks); extra bytes %.2f MB = %.2f us at 4.81 TB/s; beyond spread and bytes: %s"
            % ("", cm - fm, (cm - fm) / n, n, (4 * B * n + 16 * hits) / 1e6, bytes_us, "nothing" if beyond <= 0 else "%.2f us = %.3f us per check" % (beyond, beyond / n)))
        say("    %-7s cycle kernels: %s" % ("", "the same in both calls: " + ", ".join(sorted(names["script"])) if names["script"] == names["follow"]
                                           else "follow %s | script %s" % (sorted(names["follow"]), sorted(names["script"]))))
        if hits != hits_f:
            findings.append("%s, s = %d: the follow reached %d steps, the script %d -- the two calls did not do the same work" % (form, s, hits_f, hits))
        if beyond > 0:
            findings.append("%s, s = %d: %.3f us per check beyond the follow's spread and the extra bytes" % (form, s, beyond / n))
    eng.close()
    say()

if args.follow_only:
    print(json.dumps(of_follow))
    sys.exit(0)

say("FINDINGS" if findings else "FINDINGS: none -- every difference lies inside the follow's own spread plus the time of the extra bytes")
for x in findings:
    say("    " + x)
if findings:
    say("    What the excess is made of is not measured here.  script_kernel<T> reads kind beside next and len, decides between two rules per arm,")
    say("    stores one quad more per advancing lane, and otherwise has the list checks' kernel boundary and one atomic add per wave.")
say()

say("the follow calls alone on the PARENT build, same session, a process of its own (--follow-only --root): medians of %d periods, %d series" % (R, args.series))
if args.parent_root is None:
    say("    not measured (no --parent-root)")
else:
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--follow-only", "--root", args.parent_root, "--reps", str(R), "--series", str(args.series)],
                       cwd=args.parent_root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        say("    FAILED (exit %d); nothing further is started" % p.returncode)
        args.parent_root = None
    else:
        for k, v in json.loads(line[-1]).items():
            mine = of_follow[k]
            say("    %-12s parent %s -> %9.2f (spread %.2f)   this build -> %9.2f" % (k, " ".join("%9.2f" % x for x in v), np.median(v), max(v) - min(v), np.median(mine)))
say()

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
say()

say("(f) tools/isa_diff.py, parent against this build")
if args.isa_diff is None or not os.path.exists(args.isa_diff):
    say("    not recorded (no --isa-diff)")
else:
    for ln in open(args.isa_diff).read().splitlines():
        say("    " + ln)

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(L) + "\n")
