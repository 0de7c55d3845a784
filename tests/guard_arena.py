"""Guarded device arrays: one allocation from which a test carves every array it hands to the library, with bands of known bytes
in front of and behind each, so that a store or a read outside a caller's array shows instead of falling into allocator slack.

A helper of the suite like hp_reference.py, not a conftest.py: tests/test_guard_arena.py proves on CPU tensors that it catches what it
is for, tests/test_gpu_extents.py runs every entry point that takes a caller's device array on arrays carved here.

The arena.  ``Arena(device, seed)`` owns one ``torch.uint8`` tensor.  ``carve(name, shape, dtype, role, skew)`` returns a contiguous
typed view of it.  ``skew=0`` starts the view on a 16-byte boundary, ``skew=1`` one element behind one -- allowed only for arguments
whose alignment rule in include/vfik.h is the element type; the arguments the header wants 16-byte aligned (ALIGN16) stay at 0.

The bands.  Every region has BAND = 16 KiB in front of it and behind it that belong to nobody else.  The size follows from the code:
the largest run of stores one wave issues for one output is a tile of 64 rows of 16 doubles (a pose row), 64 * 16 * 8 = 8 KiB; the
band is twice that, so a whole tile placed one wave too far, in either direction, still lands in bytes the test owns.  No read or
write of a kernel that is wrong by up to a tile can leave the allocation: the test reports, it cannot fault.

The fill.  Every byte of the arena starts as ``numpy.random.default_rng(seed).bytes(capacity)[offset]``: it depends on where it is, so
a stray copy of another part of the arena differs from what belongs there.  Output regions start with the same fill (rows a call
leaves alone must keep it); a region carved at skew=1 starts with the bytes of its skew-0 place, and the layout of the regions behind
it does not depend on the skew, so the runs of one case at both skews start from the same arrays.  The bands next to a ``role="in"``
region take one of two fills instead, chosen per arena: ``"nan"``, every byte 0xFF (NaN as float32 and as float64, -1 as int32), or ``"huge"``, every byte 0x7F (3.39e38 / 1.38e306, a large positive
int32).  A result that depends on bytes behind the end of an input differs between the two.

The check.  ``damaged()`` returns one record per band whose bytes changed -- region, side, first and last changed offset relative to
the region's edge (behind: 0 is the first byte behind the end; front: -1 is the last byte in front of the start), count -- and one
per input region that was written to (side "inside").  Empty: all intact.  ``plain_copy(name)`` is a tensor allocated on its own with
the region's initial bytes: the comparison run's array.

One limit: a store that writes exactly the bytes already there cannot be seen.  The position-dependent fill makes that a 1-in-256
chance per byte for a store of anything but the arena's own bytes at that very place."""
import numpy as np

BAND = 16384
TILE_BYTES = 64 * 16 * 8          # the largest run of stores of one wave for one output: 64 rows of 16 doubles
assert BAND == 2 * TILE_BYTES
FILLS = {"nan": 0xFF, "huge": 0x7F}
# arguments include/vfik.h wants 16-byte aligned (vfik_follow / vfik_script: way16; vfik_link_points: rep4; vfik_link_clearance and
# vfik_link_avoid: pts4; vfik_set_coupling: link_traj, whose rows are the rep4 of the blocks' vfik_link_points); every other device array
# is aligned to its element type
ALIGN16 = frozenset(("way16", "rep4", "pts4", "link_traj"))


def _round16(x):
    return (x + 15) & ~15


class Region:
    __slots__ = ("name", "arg", "shape", "dtype", "role", "skew", "start", "nbytes", "front", "back", "view")

    @property
    def end(self):
        return self.start + self.nbytes


class Arena:
    def __init__(self, device="cpu", seed=0, fill="nan", capacity=1 << 20):
        import torch
        if fill not in FILLS:
            raise ValueError("fill must be one of %s, got %r" % (sorted(FILLS), fill))
        self.device, self.seed, self.fill, self.capacity = device, int(seed), fill, int(capacity)
        self.regions = {}
        self._cursor = 0
        # what every byte held before the call under test: the fill, then whatever put() stored
        self._fill = np.frombuffer(np.random.default_rng(self.seed).bytes(self.capacity), dtype=np.uint8)
        self._init = self._fill.copy()
        raw = torch.empty(self.capacity + 16, dtype=torch.uint8, device=device)
        off = -raw.data_ptr() % 16
        self.buf = raw[off:off + self.capacity]
        assert self.buf.data_ptr() % 16 == 0
        self.buf.copy_(torch.from_numpy(self._init))

    # -- layout ------------------------------------------------------------------------------------------------------------
    def carve(self, name, shape, dtype, role, skew=0, arg=None):
        """A contiguous view of ``shape`` and ``dtype`` (a NumPy dtype or its name) between two bands of its own.  ``role``: "in" (the
        library reads it; fill it with :meth:`put`) or "out" (the library writes it; it starts with the arena's fill).  ``arg``: the
        argument's name in include/vfik.h where it differs from ``name`` -- what decides whether ``skew=1`` is allowed."""
        import torch
        if name in self.regions:
            raise ValueError("region %r is carved already" % name)
        if role not in ("in", "out"):
            raise ValueError("role must be 'in' or 'out', got %r" % (role,))
        if skew not in (0, 1):
            raise ValueError("skew must be 0 or 1, got %r" % (skew,))
        arg = arg or name
        if skew and arg in ALIGN16:
            raise ValueError("%s must be 16-byte aligned (include/vfik.h): it cannot be carved at skew=1" % arg)
        dt = np.dtype(dtype)
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        r = Region()
        r.name, r.arg, r.shape, r.dtype, r.role, r.skew = name, arg, shape, dt, role, skew
        r.nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        if r.nbytes < 1:
            raise ValueError("region %r is empty" % name)
        front0 = self._cursor                                  # (a multiple of 16)
        r.start = front0 + BAND + skew * dt.itemsize
        r.front = (r.start - BAND, r.start)
        r.back = (r.end, r.end + BAND)
        cursor = front0 + BAND + _round16(r.nbytes + 16) + BAND      # the same at both skews: every later region keeps its place
        assert r.back[1] <= cursor
        if cursor > self.capacity:
            raise ValueError("arena of %d bytes is full: region %r needs up to offset %d" % (self.capacity, name, cursor))
        self._cursor = cursor
        if skew:   # the region's own bytes are those of its skew-0 place: the runs at both skews start from the same array
            self._store(r.start, self._fill[r.start - skew * dt.itemsize:r.end - skew * dt.itemsize])
        if role == "in":
            for a, b in (r.front, r.back):
                self._store(a, np.full(b - a, FILLS[self.fill], dtype=np.uint8))
        r.view = self.buf[r.start:r.end].view(getattr(torch, dt.name)).reshape(shape)
        self.regions[name] = r
        return r.view

    def _store(self, at, bytes_):
        import torch
        self._init[at:at + len(bytes_)] = bytes_
        self.buf[at:at + len(bytes_)].copy_(torch.from_numpy(np.array(bytes_, dtype=np.uint8)))

    def put(self, name, array):
        """Store an input's values; they become the region's initial bytes (what plain_copy() hands out and damaged() holds it to)."""
        r = self.regions[name]
        a = np.ascontiguousarray(array, dtype=r.dtype)
        if a.shape != r.shape:
            raise ValueError("%s is %s, got %s" % (name, r.shape, a.shape))
        self._store(r.start, a.reshape(-1).view(np.uint8))
        return r.view

    def plain_copy(self, name):
        """A tensor allocated on its own that holds the region's initial bytes, 16-byte aligned.  The allocation has a margin of BAND
        bytes on either side (nobody checks it): in the comparison run, too, no access of a kernel that is wrong by a tile leaves memory
        the test owns."""
        import torch
        r = self.regions[name]
        raw = torch.empty(r.nbytes + 2 * BAND + 16, dtype=torch.uint8, device=self.device)
        at = BAND + (-(raw.data_ptr() + BAND) % 16)
        t = raw[at:at + r.nbytes]
        t.copy_(torch.from_numpy(self._init[r.start:r.end].copy()))
        return t.view(getattr(torch, r.dtype.name)).reshape(r.shape)

    # -- reading back ------------------------------------------------------------------------------------------------------
    def snapshot(self):
        """The carved part of the arena as it is now, on the host: what bytes_of() and damaged() read."""
        return self.buf[:self._cursor].cpu().numpy()

    def bytes_of(self, name, now=None):
        """The region's bytes as they are now: uint8 (nbytes,)."""
        r = self.regions[name]
        return (self.snapshot() if now is None else now)[r.start:r.end].copy()

    def initial_bytes(self, name):
        r = self.regions[name]
        return self._init[r.start:r.end].copy()

    def band_bytes(self):
        """Bytes damaged() looks at: both bands of every region and the inside of every input."""
        return sum(2 * BAND + (r.nbytes if r.role == "in" else 0) for r in self.regions.values())

    def damaged(self):
        """One record per band whose bytes changed, and per input region that was written: dicts with ``region``, ``side`` ("front",
        "behind" or "inside"), ``first`` and ``last`` (offsets of the first and last changed byte relative to the region's edge: behind,
        0 is the first byte behind the end; front, -1 is the last byte in front of the start; inside, 0 is the region's first byte) and
        ``count``.  Empty when everything is intact."""
        now = self.snapshot()
        out = []
        for r in self.regions.values():
            spans = [("front", r.front, r.start), ("behind", r.back, r.end)]
            if r.role == "in":
                spans.insert(1, ("inside", (r.start, r.end), r.start))
            for side, (a, b), edge in spans:
                ch = np.flatnonzero(now[a:b] != self._init[a:b])
                if ch.size:
                    out.append({"region": r.name, "side": side, "first": int(ch[0]) + a - edge, "last": int(ch[-1]) + a - edge,
                                "count": int(ch.size)})
        return out


def capacity_for(specs):
    """The arena size that holds regions of these (shape, dtype) pairs."""
    return sum(2 * BAND + _round16(int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize + 16) for shape, dt in specs)


def raw_bytes(t):
    """A tensor's bytes, uint8 (nbytes,) on the host: what the byte-for-byte comparisons compare."""
    return t.detach().contiguous().cpu().numpy().reshape(-1).view(np.uint8).copy()


def describe(records):
    return "; ".join("%(region)s %(side)s: %(count)d bytes changed, offsets %(first)d..%(last)d" % r for r in records) or "intact"


# ---- the coverage table ------------------------------------------------------------------------------------------------------
# Every vfik_* function include/vfik.h declares is in exactly one of the two (tests/test_guard_arena.py).  GUARDED: entry point -> the
# tests of tests/test_gpu_extents.py that run it on carved arrays.  EXEMPT: entry point -> why it takes no carved array.
_STEP = ("test_cycle_variants_stay_inside_the_callers_arrays",)
_MOVES = ("test_timed_moves_stay_inside_the_callers_arrays",)
_RULES = ("test_timed_moves_with_every_rule_stay_inside_the_callers_arrays",)
GUARDED = {
    "vfik_step": _STEP,
    "vfik_rollout": _STEP,
    "vfik_link_points": ("test_link_points_extents",),
    "vfik_link_clearance": ("test_link_clearance_extents",),
    "vfik_link_avoid": ("test_link_avoid_extents",),
    "vfik_track_error": ("test_track_error_extents",),
    "vfik_probe_field": ("test_probe_field_extents",),
    "vfik_object_distances": ("test_object_distances_extents",),
    "vfik_mix": ("test_mix_extents",),
    "vfik_move_fields": ("test_move_fields_extents",),
    "vfik_move_scene": ("test_move_scene_extents",),
    "vfik_goto": _MOVES + _RULES,
    "vfik_follow": _MOVES + _RULES,
    "vfik_goto_js": _MOVES + _RULES,
    "vfik_follow_js": _MOVES + _RULES,
    "vfik_script": _MOVES + _RULES,
    # the rules' device arrays are the caller's and are read and written by the moves that follow
    "vfik_set_stall_rule": _RULES,
    "vfik_set_coupling": _RULES,
    "vfik_set_wait_rule": _RULES,
    "vfik_set_avoid_rule": _RULES,
}
_HOST = "a host-pointer form: it stages through the handle's own device buffers and hands no caller's device array to a kernel"
_SETTER = "a setter: it copies host values into the handle's own images"
_QUERY = "a query: it returns a value of the handle or the library and touches no caller's device array"
_MEM = "a memory helper: it allocates, frees or copies whole buffers by the size the caller gives"
EXEMPT = dict(
    [(k, _HOST) for k in ("vfik_step_host", "vfik_rollout_host", "vfik_submit_host", "vfik_wait", "vfik_goto_host", "vfik_follow_host",
                          "vfik_goto_js_host", "vfik_follow_js_host", "vfik_script_host", "vfik_move_fields_host", "vfik_move_scene_host",
                          "vfik_link_points_host", "vfik_link_clearance_host", "vfik_link_avoid_host", "vfik_stalled_host",
                          "vfik_waited_host")]
    + [(k, _SETTER) for k in ("vfik_create", "vfik_destroy", "vfik_set_stream", "vfik_set_chain", "vfik_set_params", "vfik_set_tool",
                              "vfik_set_speed_scale", "vfik_set_fields", "vfik_set_mixer_weights", "vfik_set_ext_cmd", "vfik_reset_state",
                              "vfik_track_reset", "vfik_set_link_spheres", "vfik_set_arm_weights", "vfik_set_max_vel", "vfik_set_objects",
                              "vfik_set_small_batch_kernel")]
    + [(k, _QUERY) for k in ("vfik_abi_version", "vfik_struct_sizes", "vfik_last_error", "vfik_device_count", "vfik_supported_joints",
                             "vfik_sync", "vfik_scene_move_size", "vfik_goto_opts_size", "vfik_follow_opts_size", "vfik_goto_js_opts_size",
                             "vfik_follow_js_opts_size", "vfik_script_opts_size", "vfik_stall_rule_size", "vfik_link_sphere_size",
                             "vfik_coupling_size", "vfik_wait_rule_size", "vfik_avoid_rule_size", "vfik_slots_in_use", "vfik_field_path",
                             "vfik_uniform_repellers", "vfik_one_chunk", "vfik_mixed_orders", "vfik_launch_epoch", "vfik_dh_pattern",
                             "vfik_device_bytes", "vfik_small_batch_launches", "vfik_launched_kernels")]
    + [(k, _MEM) for k in ("vfik_dev_alloc", "vfik_dev_free", "vfik_memcpy_h2d", "vfik_memcpy_d2h", "vfik_host_alloc", "vfik_host_free")]
    + [("vfik_time_steps", "a query of launch time: it enqueues vfik_step's own launch on the same io, which the step cases guard")])
