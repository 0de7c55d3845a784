"""Batch sharding across the GPUs of a node.

Every arm is an independent problem (the reference runs one process set per arm,
/root/reference/scripts/vfclik:88-105), so the batch splits into contiguous slices, one per rank,
and the control path needs no collective.  ``collate`` is the optional gather of per-rank results
into one array (one all_gather; RCCL over xGMI on GPUs, gloo in the CPU tests).
"""


def shard_range(batch, rank, world):
    """Contiguous slice [lo, hi) of rank ``rank``: sizes differ by at most one, lower ranks first."""
    if not (0 <= rank < world):
        raise ValueError("rank %d outside world %d" % (rank, world))
    base, extra = divmod(int(batch), int(world))
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def shard_sizes(batch, world):
    return [shard_range(batch, r, world)[1] - shard_range(batch, r, world)[0] for r in range(world)]


def collate(local, batch, dist=None):
    """All-gather the per-rank rows (torch tensor (b_r, ...)) into the full (batch, ...) tensor on
    every rank.  Ragged shards are padded to the largest shard for the collective."""
    import torch
    if dist is None:
        import torch.distributed as dist
    world, rank = dist.get_world_size(), dist.get_rank()
    sizes = shard_sizes(batch, world)
    assert local.shape[0] == sizes[rank], "rank %d holds %d rows, expected %d" % (rank, local.shape[0], sizes[rank])
    pad = max(sizes)
    buf = torch.zeros((pad,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    buf[: local.shape[0]] = local
    parts = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(parts, buf)
    return torch.cat([p[:s] for p, s in zip(parts, sizes)], dim=0)


def _rank_world(rank, world):
    """(rank, world) of this process: explicit arguments, else an initialised torch.distributed group, else the
    launcher's environment (RANK / WORLD_SIZE), else a single process."""
    import os
    if rank is not None and world is not None:
        return int(rank), int(world)
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except ImportError:
        pass
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


class ShardedEngine:
    """A global batch of arms over the GPUs of a node: the batched analogue of scripts/vfclik:88-105, which starts
    one process set per arm.  Rank r of ``world`` (one process per GPU under torch.distributed / bench.py's own
    launcher) owns the contiguous arms ``shard_range(batch, r, world)``; inside a rank the shard is split once more over
    ``devices`` (default: the rank's LOCAL_RANK device when world > 1, every visible device in a single process), one
    ``Engine`` handle and one stream per device.  The devices of a rank work CONCURRENTLY, as the reference's per-arm
    process sets do (vfclik:88-105): a cycle is submitted to every device before the first one is waited for
    (:meth:`step_host`).  Global arrays in, the rank's rows out; ``gather`` collates the rows of all ranks (one
    all_gather, never on the control path).

    engine_factory(chain, batch, device=..., **kw) builds a handle (default ``engine.Engine``; CPU tests inject a
    stand-in -- the product has no CPU path)."""

    def __init__(self, chain, batch, rank=None, world=None, devices=None, engine_factory=None, **engine_kw):
        import os
        self.chain = chain
        self.batch = int(batch)
        self.rank, self.world = _rank_world(rank, world)
        self.lo, self.hi = shard_range(self.batch, self.rank, self.world)
        if engine_factory is None:
            from .engine import Engine as engine_factory
        if devices is None:
            if self.world > 1:
                devices = [int(os.environ.get("LOCAL_RANK", self.rank))]
            else:
                from .engine import load_library
                devices = list(range(max(1, load_library().vfik_device_count())))
        self.devices = list(devices)
        # the rank's rows over its devices: again contiguous, sizes differing by at most one; devices left without an
        # arm (more devices than arms) get no handle
        self.parts = []
        for k, dev in enumerate(self.devices):
            a, b = shard_range(self.hi - self.lo, k, len(self.devices))
            if b > a:
                self.parts.append((self.lo + a, self.lo + b, engine_factory(chain, b - a, device=dev, **engine_kw)))
        self.engines = [e for _, _, e in self.parts]
        self._pin = {}

    @property
    def local_rows(self):
        return self.hi - self.lo

    def close(self):
        for e in self.engines:
            e.close()
        self.parts, self.engines = [], []

    def local(self, arr):
        """This rank's rows of a global (batch, ...) array."""
        if arr.shape[0] != self.batch:
            raise ValueError("expected a global array of %d rows, got %d" % (self.batch, arr.shape[0]))
        return arr[self.lo:self.hi]

    def _rows(self, arr, name, global_rows):
        if arr is None:
            return [None] * len(self.parts)
        want = self.batch if global_rows else self.local_rows
        if arr.shape[0] != want:
            raise ValueError("%s: expected %d rows (%s), got %d" % (name, want, "global" if global_rows else "this rank's", arr.shape[0]))
        off = 0 if global_rows else self.lo
        return [arr[a - off:b - off] for a, b, _ in self.parts]

    def set_fields(self, fields, counts, global_rows=True):
        """Field sets of the whole batch (global_rows) or of this rank's rows only (a caller that never holds the
        global arrays, e.g. bench.py's per-rank synthetic workload)."""
        for (a, b, e), f, c in zip(self.parts, self._rows(fields, "fields", global_rows), self._rows(counts, "counts", global_rows)):
            e.set_fields(f, c)

    def move_fields_host(self, goal=None, repellers=None, global_rows=True):
        """Engine.move_fields_host over the shard: goal frames (rows, 16) and / or x y z radius (rows, n_rep, 4) of the whole
        batch (global_rows) or of this rank's rows, split as :meth:`set_fields` splits its arrays."""
        for (a, b, e), g, r in zip(self.parts, self._rows(goal, "goal", global_rows), self._rows(repellers, "repellers", global_rows)):
            e.move_fields_host(goal=g, repellers=r)

    def move_scene_host(self, goal=None, repellers=None, funnels=None, hemispheres=None, attractors=None, global_rows=True):
        """Engine.move_scene_host over the shard, every array split as :meth:`set_fields` splits its arrays."""
        given = (("goal", goal), ("repellers", repellers), ("funnels", funnels), ("hemispheres", hemispheres), ("attractors", attractors))
        split = {name: self._rows(arr, name, global_rows) for name, arr in given}
        for k, (a, b, e) in enumerate(self.parts):
            e.move_scene_host(**{name: rows[k] for name, rows in split.items()})

    # the columns of every output row (Engine._OUT_SHAPES): what a rank without a single arm still has to return
    _COLS = {"qdot_vf": "n", "qdot_null": "n", "qdot_out": "n", "pose": 16, "pose_nt": 16, "v6": 6, "qdist": "n", "goal_dist": 2,
             "q_ref_out": "n", "track_error": 8}

    def _out_arrays(self, want, into, dtype):
        """This rank's output arrays (local_rows x columns), freshly zeroed or the caller's `into` arrays, and per part the views
        of its rows: a part writes straight into its rows, nothing is concatenated afterwards."""
        import numpy as np
        full = {}
        for k in want:
            if into is not None and k in into:
                full[k] = into[k]
                if full[k].shape[0] != self.local_rows:
                    raise ValueError("into[%s]: expected %d rows (this rank's), got %d" % (k, self.local_rows, full[k].shape[0]))
            elif k == "status":
                full[k] = np.zeros(self.local_rows, dtype=np.int32)
            else:
                c = self._COLS[k]
                full[k] = np.zeros((self.local_rows, self.chain.n if c == "n" else c), dtype=dtype)
        views = [{k: v[a - self.lo:b - self.lo] for k, v in full.items()} for a, b, _ in self.parts]
        return full, views

    def _pinned(self, i, key, shape, dtype):
        """Pinned staging array of part i (Engine.host_array), kept while its shape fits: the pipelined host path is asynchronous
        only from / to pinned memory -- a copy from pageable memory blocks the submitting thread until it is done."""
        slot = self._pin.setdefault(i, {})
        arr = slot.get(key)
        if arr is None or arr.shape != tuple(shape) or arr.dtype != dtype:
            arr = slot[key] = self.engines[i].host_array(tuple(shape), dtype)
        return arr

    def step_host(self, q, null_control=None, want=("qdot_out",), global_rows=True, into=None, **kw):
        """One control cycle of this rank's arms: host arrays in (global or local rows), this rank's rows out.
        Per-arm keyword arrays of Engine.step_host (q_ref, q_cmded, active, q_lo, q_hi) are sliced the same way; `into`
        (a dict of this rank's output arrays from an earlier call) is written in place, so the rows of arms gated off by
        `active` keep their content.

        The rank's devices run concurrently, from this one thread: every part's inputs are staged into ITS pinned arrays and
        the cycle is SUBMITTED (Engine.submit_host: copy engine / kernel / copy engine on the part's own streams) to every
        device before the first one is waited for; then the outputs are copied out of the pinned arrays.  (Handles without the
        pipelined path -- the CPU tests' stand-in -- go through one thread per device around the blocking step_host.)  A rank
        that owns no arm (more ranks than arms) returns arrays of zero rows."""
        import numpy as np
        qs = self._rows(q, "q", global_rows)
        ncs = self._rows(null_control, "null_control", global_rows)
        kws = {k: self._rows(v, k, global_rows) for k, v in kw.items() if v is not None}
        dtype = getattr(self.engines[0], "io_dtype", np.float64) if self.engines else (q.dtype if hasattr(q, "dtype") else np.float64)
        full, views = self._out_arrays(tuple(want), into, dtype)
        if not self.parts:
            return full
        pipelined = all(hasattr(e, "submit_host") and hasattr(e, "host_array") for e in self.engines) and \
            set(kws) <= {"q_ref", "q_cmded", "active", "q_lo", "q_hi"} and all(k != "obj_dist" and k != "track_error" for k in want)
        if pipelined:
            tickets, staged = [], []
            gated = "active" in kws
            for i, (a, b, e) in enumerate(self.parts):           # every device gets its work ...
                args = {}
                for key, rows in [("q", qs[i]), ("null_control", ncs[i])] + [(k, v[i]) for k, v in kws.items()]:
                    if rows is None:
                        continue
                    dt = np.int32 if key == "active" else e.io_dtype
                    rows = (np.asarray(rows) != 0) if key == "active" else rows
                    pin = self._pinned(i, "in_" + key, np.shape(rows), np.dtype(dt))
                    pin[...] = rows
                    args[key] = pin
                outs = {}
                for k, v in views[i].items():
                    outs[k] = self._pinned(i, "out_" + k, v.shape, v.dtype)
                    if gated:
                        outs[k][...] = v          # rows of gated arms come back as they went in
                staged.append(outs)
                tickets.append(e.submit_host(args.pop("q"), outs, **args))
            for (a, b, e), t in zip(self.parts, tickets):        # ... before the first one is waited for
                e.wait(t)
            for outs, view in zip(staged, views):
                for k, v in view.items():
                    v[...] = outs[k]
            return full
        if len(self.parts) == 1:
            (a, b, e), = self.parts
            e.step_host(qs[0], null_control=ncs[0], want=want, into=views[0], **{k: v[0] for k, v in kws.items()})
            return full
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=len(self.parts)) as pool:
            futs = [pool.submit(e.step_host, qs[i], null_control=ncs[i], want=want, into=views[i], **{k: v[i] for k, v in kws.items()})
                    for i, (a, b, e) in enumerate(self.parts)]
            for f in futs:
                f.result()
        return full

    def goto_host(self, q, n_cycles, dt, precision, global_rows=True, **kw):
        """Engine.goto_host over this rank's arms: host arrays in (global or local rows), this rank's rows out, concatenated in arm
        order -- ``q``, ``arrived``, the rows named in ``want`` and, with ``trajectory``, ``q_traj`` / ``dist_traj`` (along their arm
        axis).  Per-arm keyword arrays (null_control, active, q_lo, q_hi, q_ref) are sliced as :meth:`step_host` slices them.  Every
        part's goto is enqueued before any is waited for: a goto with ``poll`` reads its counts back while it runs, so each device is
        driven by a thread of its own around the blocking call (the stand-in path of :meth:`step_host`), and the devices work
        concurrently.  With ``poll`` each part ends when ITS arms are there: ``checks_run`` is the largest count, ``pending`` the sum over
        the parts (a part that ended early adds 0), and the traces of a part that ended early repeat its last row."""
        qs_of = self._rows(q, "q", global_rows)
        return self._checked_host(lambda e, i, a: e.goto_host(qs_of[i], n_cycles, dt, precision, **a), global_rows, kw)

    def follow_host(self, q, way, n_cycles, dt, precision, global_rows=True, **kw):
        """Engine.follow_host over this rank's arms, as :meth:`goto_host`: ``way`` (rows, W, 16) is sharded with the arms; ``reached``,
        ``next`` and, with ``trajectory``, ``way_traj`` (along its arm axis) come back in arm order beside what :meth:`goto_host` returns."""
        import numpy as np
        qs_of, ways = self._rows(q, "q", global_rows), self._rows(np.asarray(way), "way", global_rows)
        return self._checked_host(lambda e, i, a: e.follow_host(qs_of[i], ways[i], n_cycles, dt, precision, **a), global_rows, kw)

    def goto_js_host(self, q, q_ref, n_cycles, dt, precision, global_rows=True, **kw):
        """Engine.goto_js_host over this rank's arms, as :meth:`goto_host`: ``q_ref`` is sharded with the arms, ``precision`` (one value
        per joint) is shared; ``diff`` comes back in arm order beside ``q`` and ``arrived``."""
        qs_of, refs = self._rows(q, "q", global_rows), self._rows(q_ref, "q_ref", global_rows)
        return self._checked_host(lambda e, i, a: e.goto_js_host(qs_of[i], refs[i], n_cycles, dt, precision, **a), global_rows, kw)

    def follow_js_host(self, q, wayq, n_cycles, dt, precision, global_rows=True, **kw):
        """Engine.follow_js_host over this rank's arms, as :meth:`follow_host`: ``wayq`` (rows, W, n) is sharded with the arms, ``precision``
        and ``via_precision`` are shared."""
        import numpy as np
        qs_of, ways = self._rows(q, "q", global_rows), self._rows(np.asarray(wayq), "wayq", global_rows)
        return self._checked_host(lambda e, i, a: e.follow_js_host(qs_of[i], ways[i], n_cycles, dt, precision, **a), global_rows, kw)

    def script_host(self, q, kind, way, wayq, n_cycles, dt, precision, js_precision, global_rows=True, **kw):
        """Engine.script_host over this rank's arms, as :meth:`follow_host`: ``kind`` (rows, W), ``way`` (rows, W, 16) and ``wayq``
        (rows, W, n) are sharded with the arms; the precisions and the two mixer quads are shared."""
        import numpy as np
        qs_of, kinds = self._rows(q, "q", global_rows), self._rows(np.asarray(kind), "kind", global_rows)
        ways, wayqs = self._rows(np.asarray(way), "way", global_rows), self._rows(np.asarray(wayq), "wayq", global_rows)
        return self._checked_host(lambda e, i, a: e.script_host(qs_of[i], kinds[i], ways[i], wayqs[i], n_cycles, dt, precision, js_precision, **a),
                                  global_rows, kw)

    def set_stall_rule(self, patience, eps=(0.0, 0.0), eps_js=0.0, stop=True):
        """Engine.set_stall_rule on every engine of this rank (``patience=None``: off); each engine keeps its own ``stalled`` array.  While
        the rule is set the host forms return ``stalled`` in arm order beside their other per-arm rows."""
        for e in self.engines:
            e.set_stall_rule(patience, eps=eps, eps_js=eps_js, stop=stop)

    def stalled(self):
        """Engine.stalled of this rank's arms, in arm order."""
        import numpy as np
        return np.concatenate([e.stalled() for e in self.engines], axis=0)

    # -- arms as each other's obstacles: a source arm must live on the engine of the arm it is an obstacle for -----------------------------
    def set_link_spheres(self, spheres):
        """Engine.set_link_spheres on every engine of this rank: the spheres sit on the chain's links, the same for every arm."""
        for e in self.engines:
            e.set_link_spheres(spheres)

    def _local_sources(self, src_arm, global_rows):
        """src_arm in GLOBAL arm indices (global or this rank's rows) -> per part the indices inside that part's engine; None: every arm
        its own source.  A negative index stays (no source).  ValueError when an arm's source lies on another engine: there is no
        plumbing between handles (include/vfik.h: vfik_link_points)."""
        import numpy as np
        if src_arm is None:
            return [None] * len(self.parts)
        out = []
        for (a, b, _), rows in zip(self.parts, self._rows(np.asarray(src_arm), "src_arm", global_rows)):
            rows = np.asarray(rows, dtype=np.int64)
            away = (rows >= 0) & ((rows < a) | (rows >= b))
            if away.any():
                k = int(np.flatnonzero(away)[0])
                raise ValueError("arm %d: its source arm %d lies in another shard (this one holds arms %d..%d)" % (a + k, rows[k], a, b - 1))
            out.append(np.where(rows >= 0, rows - a, rows).astype(np.int32))
        return out

    def link_points_host(self, q, src_arm=None, xform=None, n_rep=None, first_rep=0, global_rows=True):
        """Engine.link_points_host over this rank's arms: ``q`` (rows, n) and ``xform`` (rows, 12) are sharded with the arms, ``src_arm``
        (rows,) holds GLOBAL arm indices and is translated per shard.  Returns this rank's rows (local_rows, n_rep, 4) in arm order."""
        import numpy as np
        srcs = self._local_sources(src_arm, global_rows)
        qs = self._rows(np.asarray(q), "q", global_rows)
        xs = self._rows(None if xform is None else np.asarray(xform).reshape(len(xform), 12), "xform", global_rows)
        outs = [e.link_points_host(qs[i], srcs[i], xs[i], n_rep=n_rep, first_rep=first_rep) for i, e in enumerate(self.engines)]
        return np.concatenate(outs, axis=0) if outs else np.zeros((0, n_rep or 0, 4))

    def set_coupling(self, src_arm=None, xform=None, first_rep=0, trace_checks=None, global_rows=True):
        """Engine.set_coupling on every engine of this rank; ``src_arm`` in GLOBAL arm indices, ``xform`` sharded with the arms, both
        host arrays; ``trace_checks``: None or the number of checks every engine keeps a trace of (:meth:`link_traj`).
        ``set_coupling(None)`` switches the coupling off."""
        import numpy as np
        if src_arm is None and xform is None and trace_checks is None:
            for e in self.engines:
                e.set_coupling(None)
            return
        srcs = self._local_sources(src_arm, global_rows)   # (None: every arm its own source, on whichever engine it lives)
        xs = self._rows(None if xform is None else np.asarray(xform).reshape(len(xform), 12), "xform", global_rows)
        for i, e in enumerate(self.engines):
            e.set_coupling(src_arm=srcs[i], xform=xs[i], first_rep=first_rep, trace_checks=trace_checks)

    def link_traj(self):
        """Engine.link_traj of this rank's arms, along their arm axis."""
        import numpy as np
        return np.concatenate([e.link_traj() for e in self.engines], axis=1)

    # -- clearance and the wait rule: per arm, so the one cross-shard case is the source arm that set_coupling refuses already ------------
    def link_clearance_host(self, q, points, first=0, count=None, mask=None, global_rows=True):
        """Engine.link_clearance_host over this rank's arms: ``q`` (rows, n) and ``points`` (rows, n_rep, 4) are sharded with the arms.
        Returns this rank's ``(clear, pair)`` in arm order."""
        import numpy as np
        qs = self._rows(np.asarray(q), "q", global_rows)
        ps = self._rows(np.asarray(points), "points", global_rows)
        outs = [e.link_clearance_host(qs[i], ps[i], first=first, count=count, mask=mask) for i, e in enumerate(self.engines)]
        if not outs:
            return np.zeros(0), np.zeros(0, dtype=np.int32)
        return np.concatenate([o[0] for o in outs], axis=0), np.concatenate([o[1] for o in outs], axis=0)

    def set_wait_rule(self, min_clearance, yields=None, mask=None, trace_checks=None, global_rows=True):
        """Engine.set_wait_rule on every engine of this rank (``min_clearance=None``: off); ``yields`` (rows,) is a host array sharded with
        the arms.  Each engine keeps its own ``waited`` array and, with ``trace_checks``, its own traces.  While the rule is set the host
        forms return ``waited`` in arm order beside their other per-arm rows."""
        import numpy as np
        ys = self._rows(None if yields is None else np.asarray(yields), "yields", global_rows)
        for i, e in enumerate(self.engines):
            e.set_wait_rule(min_clearance, yields=ys[i], mask=mask, trace_checks=trace_checks)

    def waited(self):
        """Engine.waited of this rank's arms, in arm order."""
        import numpy as np
        return np.concatenate([e.waited() for e in self.engines], axis=0)

    # -- whole-arm avoidance: per arm like the wait rule ----------------------------------------------------------------------------------
    def link_avoid_host(self, q, points, first=0, count=None, mask=None, gain=1.0, d0=0.1, scale=None, global_rows=True):
        """Engine.link_avoid_host over this rank's arms: ``q`` (rows, n), ``points`` (rows, n_rep, 4) and ``scale`` (rows,) are sharded
        with the arms.  Returns this rank's commands (rows, n) in arm order."""
        import numpy as np
        qs = self._rows(np.asarray(q), "q", global_rows)
        ps = self._rows(np.asarray(points), "points", global_rows)
        ss = self._rows(None if scale is None else np.asarray(scale), "scale", global_rows)
        outs = [e.link_avoid_host(qs[i], ps[i], first=first, count=count, mask=mask, gain=gain, d0=d0, scale=ss[i])
                for i, e in enumerate(self.engines)]
        return np.concatenate(outs, axis=0) if outs else np.zeros((0, 0))

    def set_avoid_rule(self, gain, d0=None, channel=4, scale=None, mask=None, trace_checks=None, global_rows=True):
        """Engine.set_avoid_rule on every engine of this rank (``gain=None``: off); ``scale`` (rows,) is a host array sharded with the
        arms.  With ``trace_checks`` each engine keeps its own trace (:meth:`avoid_traj`)."""
        import numpy as np
        ss = self._rows(None if scale is None else np.asarray(scale), "scale", global_rows)
        for i, e in enumerate(self.engines):
            e.set_avoid_rule(gain, d0, channel=channel, scale=ss[i], mask=mask, trace_checks=trace_checks)

    def avoid_traj(self):
        """Engine.avoid_traj of this rank's arms: (n_checks, rows, n) in arm order."""
        import numpy as np
        return np.concatenate([e.avoid_traj() for e in self.engines], axis=1)

    def _checked_host(self, run, global_rows, kw):
        """``run(engine, part, keywords)`` -- an Engine.goto_host or Engine.follow_host on the part's rows -- for every part of this rank,
        each on a thread of its own, and the parts' results put together in arm order."""
        import numpy as np
        per_arm = ("null_control", "active", "q_lo", "q_hi", "q_ref")
        kws = {k: self._rows(kw.pop(k), k, global_rows) for k in per_arm if kw.get(k) is not None}
        for k in per_arm:
            kw.pop(k, None)
        if not self.parts:
            raise ValueError("this rank owns no arm: there is nothing to drive")

        def one(i):
            return run(self.engines[i], i, dict(kw, **{k: v[i] for k, v in kws.items()}))
        if len(self.parts) == 1:
            return one(0)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=len(self.parts)) as pool:
            outs = list(pool.map(one, range(len(self.parts))))
        ran = max(o["checks_run"] for o in outs)
        full = {"checks_run": ran}
        for k in outs[0]:
            if k == "checks_run":
                continue
            if k == "pending":
                full[k] = np.sum([np.pad(o[k], (0, ran - len(o[k]))) for o in outs], axis=0).astype(np.int32)
            elif k in ("q_traj", "dist_traj", "way_traj"):
                full[k] = np.concatenate([np.concatenate([o[k]] + [o[k][-1:]] * (ran - len(o[k])), axis=0) for o in outs], axis=1)
            else:
                full[k] = np.concatenate([o[k] for o in outs], axis=0)
        return full

    def gather(self, local_rows, dist=None):
        """The rows of every rank, in arm order, on every rank (torch tensor in, torch tensor out)."""
        if self.world == 1:
            return local_rows
        return collate(local_rows, self.batch, dist)

    def step_global(self, q, want=("qdot_out",), dist=None, **kw):
        """step_host on this rank's rows of the global q, then the collated global rows of every output."""
        import torch
        out = self.step_host(q, want=want, **kw)
        return {k: self.gather(torch.from_numpy(v), dist).numpy() for k, v in out.items()}
