"""ctypes binding of libvfik_hip.so (include/vfik.h) -- the only compute path of this package.

``Engine`` owns one ``vfik_handle``: the batched state of the reference's per-arm vf / nullspace /
debug_jointlimits / bridge-mixer processes on one GPU.  It fails loudly when the HIP library is
missing or no GPU is visible; nothing here computes on the CPU.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from .chain import Chain


class VfikError(RuntimeError):
    pass


class IO(C.Structure):
    _fields_ = [("q", C.c_void_p), ("null_control", C.c_void_p), ("qdot_vf", C.c_void_p), ("qdot_null", C.c_void_p),
                ("qdot_out", C.c_void_p), ("pose", C.c_void_p), ("pose_nt", C.c_void_p), ("v6", C.c_void_p),
                ("qdist", C.c_void_p), ("status", C.c_void_p), ("goal_dist", C.c_void_p),
                ("q_ref", C.c_void_p), ("q_cmded", C.c_void_p),
                ("active", C.c_void_p), ("q_lo", C.c_void_p), ("q_hi", C.c_void_p), ("q_ref_out", C.c_void_p),
                ("track_error", C.c_void_p), ("obj_dist", C.c_void_p)]


# columns of the members of IO as (batch, columns) arrays of the engine's dtype ("n": the chain's joints); active and status are int32
# (batch,), obj_dist is (batch, n_objects, 2): Engine._make_specs
_IN_SHAPES = {"q": "n", "null_control": _abi.NULL_CONTROLS, "q_ref": "n", "q_cmded": "n", "q_lo": "n", "q_hi": "n"}
_OUT_SHAPES = {"qdot_vf": "n", "qdot_null": "n", "qdot_out": "n", "pose": 16, "pose_nt": 16, "v6": 6, "qdist": "n",
               "goal_dist": 2, "q_ref_out": "n", "track_error": 8}
_lib = None


def load_library(path=None):
    """Load libvfik_hip.so and declare the prototypes of include/vfik.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("VFIK_HIP_LIB") or _abi.HIP_LIB_PATH
    try:
        # torch ships its own libamdhip64; let it load first so that this process holds ONE HIP
        # runtime (loading /opt/rocm's copy first makes a later torch.cuda init fail)
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise VfikError("HIP library %s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(there is no CPU fallback)" % path)
    lib = C.CDLL(path)
    H = C.c_void_p
    protos = {
        "vfik_abi_version": (C.c_int, []),
        "vfik_struct_sizes": (None, [C.POINTER(C.c_size_t)]),
        "vfik_last_error": (C.c_char_p, []),
        "vfik_device_count": (C.c_int, []),
        "vfik_supported_joints": (C.c_uint32, []),
        "vfik_create": (H, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "vfik_destroy": (None, [H]),
        "vfik_set_stream": (C.c_int, [H, C.c_void_p]),
        "vfik_set_chain": (C.c_int, [H, C.POINTER(_abi.Chain)]),
        "vfik_set_params": (C.c_int, [H, C.POINTER(_abi.Params)]),
        "vfik_set_tool": (C.c_int, [H, C.c_void_p, C.c_int]),
        "vfik_set_speed_scale": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p]),
        "vfik_set_fields": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
        "vfik_move_fields": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "vfik_move_fields_host": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
        "vfik_scene_move_size": (C.c_size_t, []),
        "vfik_move_scene": (C.c_int, [H, C.c_int, C.c_int, C.POINTER(_abi.SceneMove)]),
        "vfik_move_scene_host": (C.c_int, [H, C.c_int, C.c_int, C.POINTER(_abi.SceneMove)]),
        "vfik_set_mixer_weights": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p]),
        "vfik_set_ext_cmd": (C.c_int, [H, C.c_int, C.c_void_p]),
        "vfik_reset_state": (C.c_int, [H]),
        "vfik_step": (C.c_int, [H, C.POINTER(IO)]),
        "vfik_step_host": (C.c_int, [H, C.POINTER(IO)]),
        "vfik_sync": (C.c_int, [H]),
        "vfik_rollout": (C.c_int, [H, C.POINTER(IO), C.c_int, C.c_double, C.c_int, C.c_void_p]),
        "vfik_rollout_host": (C.c_int, [H, C.POINTER(IO), C.c_int, C.c_double, C.c_int, C.c_void_p]),
        "vfik_goto_opts_size": (C.c_size_t, []),
        "vfik_goto": (C.c_int, [H, C.POINTER(IO), C.POINTER(_abi.GotoOpts)]),
        "vfik_goto_host": (C.c_int, [H, C.POINTER(IO), C.POINTER(_abi.GotoOpts), C.c_int, C.POINTER(C.c_int)]),
        "vfik_follow_opts_size": (C.c_size_t, []),
        "vfik_follow": (C.c_int, [H, C.POINTER(IO), C.POINTER(_abi.FollowOpts)]),
        "vfik_follow_host": (C.c_int, [H, C.POINTER(IO), C.POINTER(_abi.FollowOpts), C.c_int, C.POINTER(C.c_int)]),
        "vfik_goto_js_opts_size": (C.c_size_t, []),
        "vfik_goto_js": (C.c_int, [H, C.POINTER(IO), C.POINTER(_abi.GotoJsOpts)]),
        "vfik_goto_js_host": (C.c_int, [H, C.POINTER(IO), C.POINTER(_abi.GotoJsOpts), C.c_int, C.POINTER(C.c_int)]),
        "vfik_follow_js_opts_size": (C.c_size_t, []),
        "vfik_follow_js": (C.c_int, [H, C.POINTER(IO), C.POINTER(_abi.FollowJsOpts)]),
        "vfik_follow_js_host": (C.c_int, [H, C.POINTER(IO), C.POINTER(_abi.FollowJsOpts), C.c_int, C.POINTER(C.c_int)]),
        "vfik_script_opts_size": (C.c_size_t, []),
        "vfik_script": (C.c_int, [H, C.POINTER(IO), C.POINTER(_abi.ScriptOpts)]),
        "vfik_script_host": (C.c_int, [H, C.POINTER(IO), C.POINTER(_abi.ScriptOpts), C.c_int, C.POINTER(C.c_int)]),
        "vfik_stall_rule_size": (C.c_size_t, []),
        "vfik_set_stall_rule": (C.c_int, [H, C.POINTER(_abi.StallRule)]),
        "vfik_stalled_host": (C.c_int, [H, C.c_void_p]),
        "vfik_link_sphere_size": (C.c_size_t, []),
        "vfik_set_link_spheres": (C.c_int, [H, C.c_void_p, C.c_int]),
        "vfik_link_points": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
        "vfik_link_points_host": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
        "vfik_coupling_size": (C.c_size_t, []),
        "vfik_set_coupling": (C.c_int, [H, C.POINTER(_abi.Coupling)]),
        "vfik_link_clearance": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
        "vfik_link_clearance_host": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
        "vfik_wait_rule_size": (C.c_size_t, []),
        "vfik_set_wait_rule": (C.c_int, [H, C.POINTER(_abi.WaitRule)]),
        "vfik_waited_host": (C.c_int, [H, C.c_void_p]),
        "vfik_link_avoid": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                      C.c_void_p, C.c_int]),
        "vfik_link_avoid_host": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p,
                                           C.c_void_p]),
        "vfik_avoid_rule_size": (C.c_size_t, []),
        "vfik_set_avoid_rule": (C.c_int, [H, C.POINTER(_abi.AvoidRule)]),
        "vfik_mix": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "vfik_track_error": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "vfik_track_reset": (C.c_int, [H]),
        "vfik_dev_alloc": (C.c_void_p, [H, C.c_size_t]),
        "vfik_dev_free": (C.c_int, [H, C.c_void_p]),
        "vfik_memcpy_h2d": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_size_t]),
        "vfik_memcpy_d2h": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_size_t]),
        "vfik_time_steps": (C.c_int, [H, C.POINTER(IO), C.c_int, C.c_int, C.POINTER(C.c_float)]),
        "vfik_slots_in_use": (C.c_int, [H]),
        "vfik_field_path": (C.c_int, [H]),
        "vfik_uniform_repellers": (C.c_int, [H]),
        "vfik_one_chunk": (C.c_int, [H]),
        "vfik_mixed_orders": (C.c_int, [H]),
        "vfik_launch_epoch": (C.c_long, [H]),
        "vfik_dh_pattern": (C.c_int, [H]),
        "vfik_device_bytes": (C.c_size_t, [H]),
        "vfik_host_alloc": (C.c_void_p, [H, C.c_size_t]),
        "vfik_host_free": (C.c_int, [H, C.c_void_p]),
        "vfik_submit_host": (C.c_int, [H, C.POINTER(IO), C.POINTER(C.c_long)]),
        "vfik_wait": (C.c_int, [H, C.c_long]),
        "vfik_set_arm_weights": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
        "vfik_set_max_vel": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p]),
        "vfik_probe_field": (C.c_int, [H, C.c_void_p, C.c_void_p]),
        "vfik_object_distances": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
        "vfik_set_objects": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p, C.c_int]),
        "vfik_set_small_batch_kernel": (C.c_int, [H, C.c_int]),
        "vfik_small_batch_launches": (C.c_long, [H]),
        "vfik_launched_kernels": (C.c_int, [H, C.c_char_p, C.c_int]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)  # AttributeError here = the library does not match include/vfik.h
        fn.restype = res
        fn.argtypes = args
    if lib.vfik_abi_version() != _abi.ABI_VERSION:
        raise VfikError("ABI version mismatch: library %d, binding %d" % (lib.vfik_abi_version(), _abi.ABI_VERSION))
    sizes = (C.c_size_t * 4)()
    lib.vfik_struct_sizes(sizes)
    mine = [C.sizeof(_abi.Field), C.sizeof(_abi.Chain), C.sizeof(_abi.Params), C.sizeof(IO)]
    if list(sizes) != mine:
        raise VfikError("struct layout mismatch: library %s, Python mirrors %s" % (list(sizes), mine))
    if lib.vfik_scene_move_size() != C.sizeof(_abi.SceneMove):
        raise VfikError("struct layout mismatch: vfik_scene_move is %d bytes in the library, %d in the Python mirror"
                        % (lib.vfik_scene_move_size(), C.sizeof(_abi.SceneMove)))
    if lib.vfik_goto_opts_size() != C.sizeof(_abi.GotoOpts):
        raise VfikError("struct layout mismatch: vfik_goto_opts is %d bytes in the library, %d in the Python mirror"
                        % (lib.vfik_goto_opts_size(), C.sizeof(_abi.GotoOpts)))
    if lib.vfik_follow_opts_size() != C.sizeof(_abi.FollowOpts):
        raise VfikError("struct layout mismatch: vfik_follow_opts is %d bytes in the library, %d in the Python mirror"
                        % (lib.vfik_follow_opts_size(), C.sizeof(_abi.FollowOpts)))
    for name, size, mirror in (("vfik_goto_js_opts", lib.vfik_goto_js_opts_size(), _abi.GotoJsOpts),
                               ("vfik_follow_js_opts", lib.vfik_follow_js_opts_size(), _abi.FollowJsOpts),
                               ("vfik_script_opts", lib.vfik_script_opts_size(), _abi.ScriptOpts),
                               ("vfik_stall_rule", lib.vfik_stall_rule_size(), _abi.StallRule),
                               ("vfik_link_sphere", lib.vfik_link_sphere_size(), _abi.LinkSphere),
                               ("vfik_coupling", lib.vfik_coupling_size(), _abi.Coupling),
                               ("vfik_wait_rule", lib.vfik_wait_rule_size(), _abi.WaitRule),
                               ("vfik_avoid_rule", lib.vfik_avoid_rule_size(), _abi.AvoidRule)):
        if size != C.sizeof(mirror):
            raise VfikError("struct layout mismatch: %s is %d bytes in the library, %d in the Python mirror" % (name, size, C.sizeof(mirror)))
    if path == _abi.HIP_LIB_PATH or _lib is None:
        _lib = lib
    return lib


def _ptr(x):
    """Device / host address of a torch tensor, numpy array or raw int."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr()  # torch.Tensor


class Engine:
    def __init__(self, chain, batch, io_dtype=np.float32, max_slots=16, device=0, params=None):
        if not isinstance(chain, Chain):
            raise TypeError("chain must be a vfclik_amd.chain.Chain")
        self.lib = load_library()
        self.chain = chain
        self.n = chain.n
        self.batch = int(batch)
        self.io_dtype = np.dtype(io_dtype)
        if self.io_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("io_dtype must be float32 or float64")
        self.max_slots = int(max_slots)
        self.device = int(device)
        bits = 32 if self.io_dtype == np.float32 else 64
        self._pinned = []
        self.h = self.lib.vfik_create(self.device, bits, self.n, self.max_slots, self.batch)
        if not self.h:
            raise VfikError("vfik_create: " + self.lib.vfik_last_error().decode())
        self._chk(self.lib.vfik_set_chain(self.h, C.byref(chain.to_struct())))
        self.params = params if params is not None else _abi.default_params()
        self._chk(self.lib.vfik_set_params(self.h, C.byref(self.params)))
        self._torch_out = {}
        self.n_objects = 0  # object frames of the distance monitor held by the handle (set_objects)
        self._stall_rule = None  # the stall rule of the timed moves (set_stall_rule), with the caller's stalled array kept alive
        self.n_links = 0  # link spheres held by the handle (set_link_spheres)
        self._coupling = None  # the coupling of the timed moves (set_coupling): the device arrays it reads and writes, kept alive
        self._wait_rule = None  # the wait rule of the timed moves (set_wait_rule): likewise
        self._avoid_rule = None  # the avoid rule of the timed moves (set_avoid_rule): likewise
        self._make_specs()

    # -- plumbing -------------------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise VfikError("vfik error %d: %s" % (rc, self.lib.vfik_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.lib.vfik_sync(self.h)
            self._drop_coupling()
            for p in self._pinned:  # arrays handed out by host_array() die with the engine
                self.lib.vfik_host_free(self.h, C.c_void_p(p))
            self._pinned = []
            self.lib.vfik_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_stream(self, stream_ptr):
        """Launch on the caller's HIP stream (``torch.cuda.current_stream().cuda_stream``)."""
        self._chk(self.lib.vfik_set_stream(self.h, C.c_void_p(stream_ptr)))

    # -- slow-changing state (event-driven in the reference) --------------------------------------
    def set_params(self, **kw):
        for k, v in kw.items():
            k = "lambda_" if k == "lambda" else k
            if k in ("wy", "wq", "mix_w"):
                arr = getattr(self.params, k)
                for i, x in enumerate(v):
                    arr[i] = float(x)
            else:
                setattr(self.params, k, v)
        self._chk(self.lib.vfik_set_params(self.h, C.byref(self.params)))

    def set_tool(self, tool16, per_arm=False):
        t = np.ascontiguousarray(tool16, dtype=np.float64)
        if t.size != (16 * self.batch if per_arm else 16):
            raise ValueError("tool must hold 16 doubles%s" % (" per arm" if per_arm else ""))
        self._chk(self.lib.vfik_set_tool(self.h, t.ctypes.data, 1 if per_arm else 0))

    def set_speed_scale(self, values, first_arm=0):
        """Per-arm speedScale (the /max_vel value each arm's vf keeps, vf:197-207)."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        self._chk(self.lib.vfik_set_speed_scale(self.h, int(first_arm), len(v), v.ctypes.data))

    def set_fields(self, fields, counts, first_arm=0):
        f = np.ascontiguousarray(fields, dtype=_abi.FIELD_DTYPE)
        if f.ndim != 2:
            raise ValueError("fields must be (n_arms, max_fields)")
        c = np.ascontiguousarray(counts, dtype=np.int32)
        self._chk(self.lib.vfik_set_fields(self.h, int(first_arm), f.shape[0], f.ctypes.data, f.shape[1], c.ctypes.data))

    def move_fields(self, goal=None, repellers=None, active=None, first_arm=0, n_arms=None, n_rep=None):
        """Goals and obstacles that move, on the device (include/vfik.h: vfik_move_fields): asynchronous on the engine's stream, no
        host pack, no synchronisation.  ``goal``: (n_arms, 16) or (n_arms, 4, 4) row-major frames of the engine's dtype -- another
        engine's ``pose`` output as it is -- replacing rows 0-2 of each arm's goal frame; ``repellers``: (n_arms, n_rep, 4) =
        x y z radius of each arm's k-th decay repeller in ascending-id order; ``active``: int32 (n_arms,), 0 leaves the arm alone.
        A row whose first element is NaN leaves that primitive alone.  Torch tensors on this device (contiguous, shapes checked), or
        raw device addresses together with ``n_arms`` (and ``n_rep`` with ``repellers``)."""
        def tensor(x):
            return x is not None and not isinstance(x, int)
        for name, x, tail in (("goal", goal, 16), ("repellers", repellers, 4), ("active", active, 1)):
            if not tensor(x):
                continue
            if not x.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
            want = "int32" if name == "active" else self.io_dtype.name
            if str(x.dtype).split(".")[-1] != want:
                raise ValueError("%s must be %s, got %s" % (name, want, x.dtype))
            rows = x.shape[0]
            if n_arms is None:
                n_arms = rows
            per_arm = x.numel() // max(rows, 1)
            if rows != n_arms or (name != "repellers" and per_arm != tail) or (name == "repellers" and (x.dim() != 3 or x.shape[2] != 4)):
                raise ValueError("%s: shape %s does not fit %s arms" % (name, tuple(x.shape), n_arms))
            if name == "repellers":
                if n_rep is not None and n_rep != x.shape[1]:
                    raise ValueError("repellers: %d rows per arm, n_rep says %d" % (x.shape[1], n_rep))
                n_rep = x.shape[1]
        if n_arms is None:
            raise ValueError("raw addresses need n_arms")
        if repellers is not None and n_rep is None:
            raise ValueError("a raw repellers address needs n_rep")
        self._chk(self.lib.vfik_move_fields(self.h, int(first_arm), int(n_arms), C.c_void_p(_ptr(goal)), C.c_void_p(_ptr(repellers)),
                                            int(n_rep or 0), C.c_void_p(_ptr(active))))

    def move_fields_host(self, goal=None, repellers=None, first_arm=0):
        """The host form (vfik_move_fields_host): NumPy arrays of doubles, rounded to the engine's dtype exactly as ``set_fields``
        rounds the parameters; (n_arms, 16) / (n_arms, 4, 4) goal frames and / or (n_arms, n_rep, 4) x y z radius.  Synchronous."""
        g = r = None
        n_arms, n_rep = None, 0
        if goal is not None:
            g = np.ascontiguousarray(goal, dtype=np.float64)
            if g.ndim < 2 or g.size != g.shape[0] * 16:
                raise ValueError("goal must be (n_arms, 16) or (n_arms, 4, 4), got %s" % (g.shape,))
            n_arms = g.shape[0]
        if repellers is not None:
            r = np.ascontiguousarray(repellers, dtype=np.float64)
            if r.ndim != 3 or r.shape[2] != 4:
                raise ValueError("repellers must be (n_arms, n_rep, 4), got %s" % (r.shape,))
            if n_arms is not None and r.shape[0] != n_arms:
                raise ValueError("goal and repellers must cover the same arms")
            n_arms, n_rep = r.shape[0], r.shape[1]
        if n_arms is None:
            raise ValueError("give goal, repellers or both")
        self._chk(self.lib.vfik_move_fields_host(self.h, int(first_arm), n_arms, None if g is None else g.ctypes.data,
                                                 None if r is None else r.ctypes.data, n_rep))

    # -- arms as each other's obstacles: spheres on links, placed on the device (vfik_set_link_spheres, vfik_link_points, vfik_set_coupling) --
    def set_link_spheres(self, spheres):
        """Spheres fixed to links of the chain (include/vfik.h: vfik_set_link_spheres): a sequence of up to 16 ``(link, centre, radius)``
        -- ``link`` 0 (the base frame) .. n (the flange, no tool), ``centre`` three coordinates in that link's frame of the PUBLIC chain
        (``Chain.B``), ``radius`` >= 0.  ``None`` or an empty sequence: none.  A new list switches a coupling off."""
        spheres = list(spheres or ())
        arr = (_abi.LinkSphere * max(len(spheres), 1))()
        for s, (link, centre, radius) in zip(arr, spheres):
            s.link, s.radius = int(link), float(radius)
            c = np.asarray(centre, dtype=np.float64).reshape(-1)
            if c.shape != (3,):
                raise ValueError("a sphere's centre has three coordinates, got %s" % (c.shape,))
            s.c[0], s.c[1], s.c[2] = c
        self._chk(self.lib.vfik_set_link_spheres(self.h, C.cast(arr, C.c_void_p) if spheres else None, len(spheres)))
        self.n_links = len(spheres)
        self._drop_coupling()

    def link_points(self, q, src_arm=None, xform=None, out=None, n_rep=None, first_rep=0):
        """Where the link spheres of every arm's source arm are, on the device (include/vfik.h: vfik_link_points): asynchronous on the
        engine's stream.  ``q`` (batch, n) of the engine's dtype; ``src_arm`` int32 (batch,) -- arm b's obstacles are the links of arm
        ``src_arm[b]``, itself when None, and a source outside the batch gives NaN rows; ``xform`` (batch, 12) or (batch, 3, 4): where
        the source's base stands as seen from arm b's.  Rows ``first_rep .. first_rep + L - 1`` of ``out`` (batch, n_rep, 4) = x y z
        radius are written, the others are not: the shape ``move_fields(repellers=out)`` takes.  Torch tensors on this device, or raw
        addresses (then ``out`` and ``n_rep`` are required).  Without ``out`` a tensor of ``n_rep`` (default first_rep + L) rows per arm
        is made, NaN outside the rows written.  Returns ``out``."""
        B, ft = self.batch, self.io_dtype.name
        if out is None:
            import torch
            n_rep = int(first_rep) + self.n_links if n_rep is None else int(n_rep)
            out = torch.full((B, n_rep, 4), float("nan"), dtype=getattr(torch, ft), device="cuda:%d" % self.device)
        elif isinstance(out, int):
            if n_rep is None:
                raise ValueError("a raw out address needs n_rep")
        else:
            if out.dim() != 3 or out.shape[0] != B or out.shape[2] != 4 or (n_rep is not None and n_rep != out.shape[1]):
                raise ValueError("out must be (%d, n_rep, 4), got %s" % (B, tuple(out.shape)))
            n_rep = out.shape[1]
        if xform is not None and not isinstance(xform, int) and xform.numel() != B * 12:
            raise ValueError("xform must be (%d, 12) or (%d, 3, 4), got %s" % (B, B, tuple(xform.shape)))
        self._check_dev((("q", q, (B, self.n), ft), ("src_arm", src_arm, (B,), "int32"), ("xform", xform, None, ft), ("out", out, None, ft)))
        self._chk(self.lib.vfik_link_points(self.h, C.c_void_p(_ptr(q)), C.c_void_p(_ptr(src_arm)), C.c_void_p(_ptr(xform)),
                                            C.c_void_p(_ptr(out)), int(n_rep), int(first_rep)))
        return out

    def link_points_host(self, q, src_arm=None, xform=None, out=None, n_rep=None, first_rep=0):
        """The host form (vfik_link_points_host; synchronous): NumPy arrays of doubles, ``q`` and ``xform`` rounded to the engine's dtype.
        Returns float64 (batch, n_rep, 4): ``out`` with the rows ``first_rep .. first_rep + L - 1`` replaced by the engine-typed values, or
        a new array that is NaN elsewhere."""
        B = self.batch
        qh = np.ascontiguousarray(q, dtype=np.float64)
        if qh.shape != (B, self.n):
            raise ValueError("q must be (%d, %d), got %s" % (B, self.n, qh.shape))
        sh = None if src_arm is None else np.ascontiguousarray(src_arm, dtype=np.int32)
        if sh is not None and sh.shape != (B,):
            raise ValueError("src_arm must be (%d,), got %s" % (B, sh.shape))
        xh = None if xform is None else np.ascontiguousarray(xform, dtype=np.float64)
        if xh is not None and xh.size != B * 12:
            raise ValueError("xform must be (%d, 12) or (%d, 3, 4), got %s" % (B, B, xh.shape))
        if out is None:
            n_rep = int(first_rep) + self.n_links if n_rep is None else int(n_rep)
            out = np.full((B, n_rep, 4), np.nan)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.ndim == 3
                  and out.shape[0] == B and out.shape[2] == 4 and n_rep in (None, out.shape[1])):
            raise ValueError("out must be a contiguous float64 array of shape (%d, n_rep, 4)" % B)
        self._chk(self.lib.vfik_link_points_host(self.h, qh.ctypes.data, None if sh is None else sh.ctypes.data,
                                                 None if xh is None else xh.ctypes.data, out.ctypes.data, out.shape[1], int(first_rep)))
        return out

    # -- link-sphere clearance and arms that wait for room (vfik_link_clearance, vfik_set_wait_rule) --
    def _mask_words(self, mask, count):
        """A pair mask as the library reads it: uint32 (L,), bit j of word i lets own sphere i meet row j.  ``mask``: None (every pair),
        L integers, or an (L, count) array of booleans."""
        if mask is None:
            return None
        m = np.asarray(mask)
        if m.ndim == 2:
            if m.shape != (self.n_links, count):
                raise ValueError("a mask matrix must be (%d, %d): own spheres by rows, got %s" % (self.n_links, count, m.shape))
            m = (m.astype(bool).astype(np.uint64) << np.arange(count, dtype=np.uint64)[None, :]).sum(axis=1)
        if m.shape != (self.n_links,):
            raise ValueError("a mask has one word per own sphere (%d), got shape %s" % (self.n_links, m.shape))
        if np.any(m.astype(np.int64) < 0) or np.any(m.astype(np.uint64) >> np.uint64(32)):
            raise ValueError("mask words are 32 bits")
        return np.ascontiguousarray(m, dtype=np.uint32)

    def link_clearance(self, q, points, first=0, count=None, mask=None, out=None, pair=None):
        """How much room is left between every arm's own link spheres and a set of other spheres, on the device (include/vfik.h:
        vfik_link_clearance): asynchronous on the engine's stream.  ``q`` (batch, n) and ``points`` (batch, n_rep, 4) = x y z radius of the
        engine's dtype -- what :meth:`link_points` writes: a neighbour's links, the arm's own, or static obstacles; a NaN row is no
        obstacle.  Rows ``first .. first + count - 1`` are looked at (``count`` default: the rest, at most 32).  ``mask``: see
        :meth:`_mask_words`.  Returns ``(out, pair)``: (batch,) of the engine's dtype, the smallest centre distance less both radii
        (+inf: no pair; NaN: a NaN in q), and int32 (batch,), own sphere * 32 + row of the closest pair (-1: none).  Torch tensors on this
        device; ``out`` / ``pair`` are made when not given."""
        import torch
        B, ft = self.batch, self.io_dtype.name
        if points.dim() != 3 or points.shape[0] != B or points.shape[2] != 4:
            raise ValueError("points must be (%d, n_rep, 4), got %s" % (B, tuple(points.shape)))
        n_rep = points.shape[1]
        count = n_rep - int(first) if count is None else int(count)
        dev = "cuda:%d" % self.device
        if out is None:
            out = torch.empty((B,), dtype=getattr(torch, ft), device=dev)
        if pair is None:
            pair = torch.empty((B,), dtype=torch.int32, device=dev)
        self._check_dev((("q", q, (B, self.n), ft), ("points", points, None, ft), ("out", out, (B,), ft), ("pair", pair, (B,), "int32")))
        mw = self._mask_words(mask, count)
        self._chk(self.lib.vfik_link_clearance(self.h, C.c_void_p(_ptr(q)), C.c_void_p(_ptr(points)), n_rep, int(first), count,
                                               None if mw is None else mw.ctypes.data, C.c_void_p(_ptr(out)), C.c_void_p(_ptr(pair))))
        return out, pair

    def link_clearance_host(self, q, points, first=0, count=None, mask=None):
        """The host form (vfik_link_clearance_host; synchronous): NumPy arrays of doubles, rounded to the engine's dtype.  Returns
        ``(clear, pair)``: float64 (batch,) holding the engine-typed values, and int32 (batch,)."""
        B = self.batch
        qh = np.ascontiguousarray(q, dtype=np.float64)
        if qh.shape != (B, self.n):
            raise ValueError("q must be (%d, %d), got %s" % (B, self.n, qh.shape))
        ph = np.ascontiguousarray(points, dtype=np.float64)
        if ph.ndim != 3 or ph.shape[0] != B or ph.shape[2] != 4:
            raise ValueError("points must be (%d, n_rep, 4), got %s" % (B, ph.shape))
        n_rep = ph.shape[1]
        count = n_rep - int(first) if count is None else int(count)
        mw = self._mask_words(mask, count)
        clear, pair = np.empty(B, dtype=np.float64), np.empty(B, dtype=np.int32)
        self._chk(self.lib.vfik_link_clearance_host(self.h, qh.ctypes.data, ph.ctypes.data, n_rep, int(first), count,
                                                    None if mw is None else mw.ctypes.data, clear.ctypes.data, pair.ctypes.data))
        return clear, pair

    def _drop_wait_rule(self):
        if self._wait_rule is not None:
            if self._wait_rule["own"]:
                self.lib.vfik_sync(self.h)   # an enqueued move may still read and write the arrays the engine uploaded
            for p in self._wait_rule["own"]:
                self.lib.vfik_dev_free(self.h, C.c_void_p(p))
            self._wait_rule = None

    def set_wait_rule(self, min_clearance, yields=None, mask=None, trace_checks=None, clear_traj=None, pair_traj=None, waited=None):
        """Let arms wait for room inside every timed move from now on (include/vfik.h: vfik_set_wait_rule); needs a coupling
        (:meth:`set_coupling`), and goes when the coupling goes.  In front of each block every arm's clearance against its partner's
        link spheres is measured, and an arm that takes part, has ``yields[b] != 0`` (None: every arm) and less than ``min_clearance``
        of room sits the block out; it runs again once the room is back.  One arm of a pair should yield and the other not: two arms
        that both yield can wait for each other, and an arm that never gets room waits until the move's time-out.
        ``yields``: int32 (batch,) -- a torch tensor on this device or a raw address, used as it is, or a NumPy array / sequence, uploaded
        and kept alive.  ``mask``: own sphere i against partner sphere j (:meth:`_mask_words`), None: every pair.  ``clear_traj`` /
        ``pair_traj``: device arrays (n_checks, batch) of the engine's dtype / int32 that receive every block's clearance and closest
        pair; ``trace_checks=N`` instead: the engine keeps both for N checks itself (:meth:`clearance_traj`).  ``waited``: int32 (batch,)
        device array for the count of blocks each arm waited, else the engine's own (:meth:`waited`).  ``min_clearance=None`` switches
        the rule off, the default.  While a rule is set every ``*_host`` form returns a ``"waited"`` key."""
        self._chk(self.lib.vfik_set_wait_rule(self.h, None))
        self._drop_wait_rule()
        if min_clearance is None:
            return
        if trace_checks is not None and (clear_traj is not None or pair_traj is not None):
            raise ValueError("give clear_traj / pair_traj (device arrays of the caller's) or trace_checks (traces of the engine's), not both")
        B, L, ft, own = self.batch, self.n_links, self.io_dtype, []
        mw = self._mask_words(mask, L)
        if mw is not None and not mw.any():
            raise ValueError("a mask without a pair: the library reads all zeros as every pair")
        try:
            if yields is not None and not isinstance(yields, int) and not hasattr(yields, "data_ptr"):
                ya = np.ascontiguousarray(yields, dtype=np.int32)
                if ya.shape != (B,):
                    raise ValueError("yields must be (%d,), got %s" % (B, ya.shape))
                yields = self._upload(ya, own)
            n_traj = None
            if trace_checks is not None:
                n_traj = int(trace_checks)
                if n_traj < 1:
                    raise ValueError("trace_checks must be at least 1, got %d" % n_traj)
                clear_traj = self._upload(np.full((n_traj, B), np.nan, dtype=ft), own)
                pair_traj = self._upload(np.full((n_traj, B), -1, dtype=np.int32), own)
            self._check_dev((("yields", yields, (B,), "int32"), ("clear_traj", clear_traj, None, ft.name), ("pair_traj", pair_traj, None, "int32"),
                             ("waited", waited, (B,), "int32")))
            r = _abi.WaitRule()
            r.min_clearance = float(min_clearance)
            r.yields, r.clear_traj, r.pair_traj, r.waited = _ptr(yields), _ptr(clear_traj), _ptr(pair_traj), _ptr(waited)
            for i in range(L if mw is not None else 0):
                r.mask[i] = int(mw[i])
            self._chk(self.lib.vfik_set_wait_rule(self.h, C.byref(r)))
        except Exception:
            for p in own:
                self.lib.vfik_dev_free(self.h, C.c_void_p(p))
            raise
        self._wait_rule = {"own": own, "keep": (yields, clear_traj, pair_traj, waited), "n_traj": n_traj,
                           "traj": (clear_traj, pair_traj) if n_traj else None}

    def waited(self):
        """int32 (batch,): how many blocks of the last timed move each arm waited for room (vfik_waited_host; synchronises).  Needs a
        wait rule."""
        out = np.empty(self.batch, dtype=np.int32)
        self._chk(self.lib.vfik_waited_host(self.h, C.c_void_p(out.ctypes.data)))
        return out

    def clearance_traj(self):
        """The engine's own traces of a wait rule set with ``trace_checks=n_checks``: ``(clear_traj, pair_traj)``, (n_checks, batch) of
        the engine's dtype and int32 -- row k what was measured in front of block k of the last timed move (NaN / -1: a block that
        never ran).  Synchronises."""
        if self._wait_rule is None or self._wait_rule["traj"] is None:
            raise VfikError("no wait rule with traces of the engine's own: set_wait_rule(..., trace_checks=n_checks)")
        n = self._wait_rule["n_traj"]
        clear, pair = np.empty((n, self.batch), dtype=self.io_dtype), np.empty((n, self.batch), dtype=np.int32)
        self.sync()
        self.d2h(clear, self._wait_rule["traj"][0])
        self.d2h(pair, self._wait_rule["traj"][1])
        return clear, pair

    # -- whole-arm avoidance: link spheres that push their own joints (vfik_link_avoid, vfik_set_avoid_rule) --
    def link_avoid(self, q, points, first=0, count=None, mask=None, gain=1.0, d0=0.1, scale=None, out=None, channel=None):
        """A joint command that pushes every arm's own link spheres away from the spheres they are close to, on the device
        (include/vfik.h: vfik_link_avoid): asynchronous on the engine's stream.  ``q``, ``points``, ``first``, ``count`` and ``mask`` as
        in :meth:`link_clearance`.  A pair closer than ``d0`` (centre distance less both radii) pushes with ``gain * scale[b] *
        (1 - d / d0)`` along the line of centres; the pushes go through the Jacobian transpose of each sphere's point.  ``scale``:
        (batch,) of the engine's dtype or None (all ones); 0 means the arm does not give way.  ``channel`` 3..5: the command is also
        written into that mixer channel of the engine's ext buffer, which must exist (:meth:`set_ext_cmd` with a command, or
        :meth:`set_avoid_rule`) -- whose mixer weight is the caller's; an existing ext buffer takes launches off the lean kernels.
        Returns ``out``, (batch, n) of the engine's dtype: zeros for an arm without an active pair or with a NaN in q; made when not
        given."""
        import torch
        B, ft = self.batch, self.io_dtype.name
        if points.dim() != 3 or points.shape[0] != B or points.shape[2] != 4:
            raise ValueError("points must be (%d, n_rep, 4), got %s" % (B, tuple(points.shape)))
        n_rep = points.shape[1]
        count = n_rep - int(first) if count is None else int(count)
        if out is None:
            out = torch.empty((B, self.n), dtype=getattr(torch, ft), device="cuda:%d" % self.device)
        self._check_dev((("q", q, (B, self.n), ft), ("points", points, None, ft), ("scale", scale, (B,), ft), ("out", out, (B, self.n), ft)))
        mw = self._mask_words(mask, count)
        self._chk(self.lib.vfik_link_avoid(self.h, C.c_void_p(_ptr(q)), C.c_void_p(_ptr(points)), n_rep, int(first), count,
                                           None if mw is None else mw.ctypes.data, float(gain), float(d0), C.c_void_p(_ptr(scale)),
                                           C.c_void_p(_ptr(out)), -1 if channel is None else int(channel)))
        return out

    def link_avoid_host(self, q, points, first=0, count=None, mask=None, gain=1.0, d0=0.1, scale=None):
        """The host form (vfik_link_avoid_host; synchronous): NumPy arrays of doubles, rounded to the engine's dtype.  Returns float64
        (batch, n) holding the engine-typed values."""
        B = self.batch
        qh = np.ascontiguousarray(q, dtype=np.float64)
        if qh.shape != (B, self.n):
            raise ValueError("q must be (%d, %d), got %s" % (B, self.n, qh.shape))
        ph = np.ascontiguousarray(points, dtype=np.float64)
        if ph.ndim != 3 or ph.shape[0] != B or ph.shape[2] != 4:
            raise ValueError("points must be (%d, n_rep, 4), got %s" % (B, ph.shape))
        sh = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
        if sh is not None and sh.shape != (B,):
            raise ValueError("scale must be (%d,), got %s" % (B, sh.shape))
        n_rep = ph.shape[1]
        count = n_rep - int(first) if count is None else int(count)
        mw = self._mask_words(mask, count)
        out = np.empty((B, self.n), dtype=np.float64)
        self._chk(self.lib.vfik_link_avoid_host(self.h, qh.ctypes.data, ph.ctypes.data, n_rep, int(first), count,
                                                None if mw is None else mw.ctypes.data, float(gain), float(d0),
                                                None if sh is None else sh.ctypes.data, out.ctypes.data))
        return out

    def _drop_avoid_rule(self):
        if self._avoid_rule is not None:
            if self._avoid_rule["own"]:
                self.lib.vfik_sync(self.h)   # an enqueued move may still read and write the arrays the engine uploaded
            for p in self._avoid_rule["own"]:
                self.lib.vfik_dev_free(self.h, C.c_void_p(p))
            self._avoid_rule = None

    def set_avoid_rule(self, gain, d0=None, channel=4, scale=None, mask=None, trace_checks=None, avoid_traj=None):
        """Let every arm's link spheres push their own joints inside every timed move from now on (include/vfik.h:
        vfik_set_avoid_rule); needs a coupling (:meth:`set_coupling`), and goes when the coupling goes.  In front of each block the
        command of :meth:`link_avoid` against the partner's link spheres is written into mixer ``channel`` (3..5) and holds for the
        block; the channel is zeroed when the move ends.  The channel's mixer weight is the caller's (``mix_w`` of the parameters,
        :meth:`set_mixer_weights`); the parameters need ``F_MIXER``.  In a script channel 4 is the natural choice: weights 4 and 5 come
        from the arm's own row there.  ``scale``: (batch,) of the engine's dtype -- a torch tensor on this device or a raw address, used
        as it is, or a NumPy array / sequence, uploaded and kept alive.  ``mask``: own sphere i against partner sphere j, None: every
        pair.  ``avoid_traj``: a device array (n_checks, batch, n) that receives every block's command; ``trace_checks=N`` instead:
        the engine keeps it for N checks itself (:meth:`avoid_traj`).  ``gain=None`` switches the rule off, the default.  The rule
        allocates the engine's ext buffer, which takes launches off the lean kernels, as any ext command does."""
        self._chk(self.lib.vfik_set_avoid_rule(self.h, None))
        self._drop_avoid_rule()
        if gain is None:
            return
        if d0 is None:
            raise ValueError("an avoid rule needs d0, the distance at which a pair begins to push")
        if trace_checks is not None and avoid_traj is not None:
            raise ValueError("give avoid_traj (a device array of the caller's) or trace_checks (a trace of the engine's), not both")
        B, L, ft, own = self.batch, self.n_links, self.io_dtype, []
        mw = self._mask_words(mask, L)
        if mw is not None and not mw.any():
            raise ValueError("a mask without a pair: the library reads all zeros as every pair")
        try:
            if scale is not None and not isinstance(scale, int) and not hasattr(scale, "data_ptr"):
                sa = np.ascontiguousarray(scale, dtype=ft)
                if sa.shape != (B,):
                    raise ValueError("scale must be (%d,), got %s" % (B, sa.shape))
                scale = self._upload(sa, own)
            n_traj = None
            if trace_checks is not None:
                n_traj = int(trace_checks)
                if n_traj < 1:
                    raise ValueError("trace_checks must be at least 1, got %d" % n_traj)
                avoid_traj = self._upload(np.full((n_traj, B, self.n), np.nan, dtype=ft), own)
            self._check_dev((("scale", scale, (B,), ft.name), ("avoid_traj", avoid_traj, None, ft.name)))
            r = _abi.AvoidRule()
            r.gain, r.d0, r.channel = float(gain), float(d0), int(channel)
            r.scale, r.avoid_traj = _ptr(scale), _ptr(avoid_traj)
            for i in range(L if mw is not None else 0):
                r.mask[i] = int(mw[i])
            self._chk(self.lib.vfik_set_avoid_rule(self.h, C.byref(r)))
        except Exception:
            for p in own:
                self.lib.vfik_dev_free(self.h, C.c_void_p(p))
            raise
        self._avoid_rule = {"own": own, "keep": (scale, avoid_traj), "n_traj": n_traj, "traj": avoid_traj if n_traj else None}

    def avoid_traj(self):
        """The engine's own trace of an avoid rule set with ``trace_checks=n_checks``: (n_checks, batch, n) of the engine's dtype -- row k
        the command written in front of block k of the last timed move (NaN: a block that never ran).  Synchronises."""
        if self._avoid_rule is None or self._avoid_rule["traj"] is None:
            raise VfikError("no avoid rule with a trace of the engine's own: set_avoid_rule(..., trace_checks=n_checks)")
        out = np.empty((self._avoid_rule["n_traj"], self.batch, self.n), dtype=self.io_dtype)
        self.sync()
        self.d2h(out, self._avoid_rule["traj"])
        return out

    def _drop_coupling(self):
        self._drop_wait_rule()   # (the library switched the rule off with the coupling)
        self._drop_avoid_rule()  # (likewise)
        if self._coupling is not None:
            if self._coupling["own"]:
                self.lib.vfik_sync(self.h)   # an enqueued move may still read the arrays the engine uploaded
            for p in self._coupling["own"]:
                self.lib.vfik_dev_free(self.h, C.c_void_p(p))
            self._coupling = None

    def _upload(self, arr, own):
        p = self.dev_alloc(max(arr.nbytes, 16))
        own.append(p)
        self.h2d(p, arr)
        return p

    def set_coupling(self, src_arm=None, xform=None, first_rep=0, link_traj=None, trace_checks=None):
        """Couple the arms inside every timed move from now on (include/vfik.h: vfik_set_coupling): in front of each block the link spheres
        of arm ``src_arm[b]`` (-1: none), seen through ``xform[b]``, become arm b's ``first_rep``-th .. decay repellers in ascending-id
        order.  ``src_arm`` / ``xform``: torch tensors on this device or raw addresses, used as they are, or NumPy arrays / sequences,
        which are uploaded (``xform`` rounded to the engine's dtype) and kept alive by the engine.  ``link_traj``: a device array
        (n_checks, batch, L, 4) that receives the rows every block started from; ``trace_checks=N`` instead: the engine keeps such a trace
        of N checks itself, read with :meth:`link_traj`.  ``set_coupling(None)`` -- no source, no transform, no trace -- switches the
        coupling off, the default; arms that are their own sources take ``src_arm=np.arange(batch)``."""
        self._chk(self.lib.vfik_set_coupling(self.h, None))
        self._drop_coupling()
        if src_arm is None and xform is None and link_traj is None and trace_checks is None:
            if first_rep != 0:
                raise ValueError("first_rep without a source, a transform or a trace: set_coupling(None) switches the coupling off")
            return
        if link_traj is not None and trace_checks is not None:
            raise ValueError("give link_traj (a device array of the caller's) or trace_checks (a trace of the engine's), not both")
        B, L, ft, own = self.batch, self.n_links, self.io_dtype, []
        try:
            if src_arm is not None and not isinstance(src_arm, int) and not hasattr(src_arm, "data_ptr"):
                sa = np.ascontiguousarray(src_arm, dtype=np.int32)
                if sa.shape != (B,):
                    raise ValueError("src_arm must be (%d,), got %s" % (B, sa.shape))
                src_arm = self._upload(sa, own)
            if xform is not None and not isinstance(xform, int) and not hasattr(xform, "data_ptr"):
                xa = np.ascontiguousarray(xform, dtype=ft)
                if xa.size != B * 12:
                    raise ValueError("xform must be (%d, 12) or (%d, 3, 4), got %s" % (B, B, xa.shape))
                xform = self._upload(xa, own)
            n_traj = None
            if trace_checks is not None:
                n_traj = int(trace_checks)
                if n_traj < 1:
                    raise ValueError("trace_checks must be at least 1, got %d" % n_traj)
                link_traj = self._upload(np.full((n_traj, B, L, 4), np.nan, dtype=ft), own)
            self._check_dev((("src_arm", src_arm, (B,), "int32"), ("xform", xform, None, ft.name), ("link_traj", link_traj, None, ft.name)))
            c = _abi.Coupling()
            c.src_arm, c.xform12, c.link_traj, c.first_rep = _ptr(src_arm), _ptr(xform), _ptr(link_traj), int(first_rep)
            self._chk(self.lib.vfik_set_coupling(self.h, C.byref(c)))
        except Exception:
            for p in own:
                self.lib.vfik_dev_free(self.h, C.c_void_p(p))
            raise
        self._coupling = {"own": own, "keep": (src_arm, xform, link_traj), "traj": link_traj if n_traj else None, "n_traj": n_traj}

    def link_traj(self):
        """The engine's own trace of a coupling set with ``trace_checks=n_checks``: (n_checks, batch, L, 4) of the engine's dtype, row k what
        block k of the last timed move started from (NaN: a block that never ran).  Synchronises."""
        if self._coupling is None or self._coupling["traj"] is None:
            raise VfikError("no coupling with a trace of the engine's own: set_coupling(..., trace_checks=n_checks)")
        out = np.empty((self._coupling["n_traj"], self.batch, self.n_links, 4), dtype=self.io_dtype)
        self.sync()
        self.d2h(out, self._coupling["traj"])
        return out

    # (name, vfik_scene_move member, its count member, elements per row; None: one row per arm)
    _SCENE_ROWS = (("goal", "goal16", None, 16), ("repellers", "rep4", "n_rep", 4), ("funnels", "fun6", "n_fun", 6),
                   ("hemispheres", "hem6", "n_hem", 6), ("attractors", "att16", "n_att", 16))

    def move_scene(self, goal=None, repellers=None, funnels=None, hemispheres=None, attractors=None, active=None, first_arm=0, n_arms=None,
                   n_rep=None, n_fun=None, n_hem=None, n_att=None):
        """The whole scene of a moving object, on the device (include/vfik.h: vfik_move_scene): ``move_fields`` and, with the same
        rules, ``funnels`` (n_arms, n_fun, 6) = x y z ax ay az of each arm's k-th funnel, ``hemispheres`` (n_arms, n_hem, 6) =
        x y z nx ny nz of its k-th hemisphere, ``attractors`` (n_arms, n_att, 16) or (n_arms, n_att, 4, 4) = the frame of its k-th
        attractor behind the goal, all in ascending-id order.  Asynchronous on the engine's stream.  Torch tensors on this device
        (contiguous, the engine's dtype, shapes checked), or raw device addresses together with ``n_arms`` and the class's count."""
        given = {"goal": goal, "repellers": repellers, "funnels": funnels, "hemispheres": hemispheres, "attractors": attractors}
        counts = {"n_rep": n_rep, "n_fun": n_fun, "n_hem": n_hem, "n_att": n_att}
        mv = _abi.SceneMove()
        for name, member, cnt, tail in self._SCENE_ROWS + (("active", "active", None, 1),):
            x = active if name == "active" else given[name]
            if x is None:
                continue
            if not isinstance(x, int):
                if not x.is_contiguous():
                    raise ValueError("%s must be contiguous" % name)
                want = "int32" if name == "active" else self.io_dtype.name
                if str(x.dtype).split(".")[-1] != want:
                    raise ValueError("%s must be %s, got %s" % (name, want, x.dtype))
                rows = x.shape[0]
                if n_arms is None:
                    n_arms = rows
                if rows != n_arms or (cnt is None and x.numel() != rows * tail) or \
                        (cnt is not None and (x.dim() < 3 or x.numel() != rows * x.shape[1] * tail)):
                    raise ValueError("%s: shape %s does not fit %s arms" % (name, tuple(x.shape), n_arms))
                if cnt is not None:
                    if counts[cnt] is not None and counts[cnt] != x.shape[1]:
                        raise ValueError("%s: %d rows per arm, %s says %d" % (name, x.shape[1], cnt, counts[cnt]))
                    counts[cnt] = x.shape[1]
            elif cnt is not None and counts[cnt] is None:
                raise ValueError("a raw %s address needs %s" % (name, cnt))
            setattr(mv, member, _ptr(x))
        if n_arms is None:
            raise ValueError("raw addresses need n_arms")
        for cnt, v in counts.items():
            setattr(mv, cnt, int(v or 0))
        self._chk(self.lib.vfik_move_scene(self.h, int(first_arm), int(n_arms), C.byref(mv)))

    def move_scene_host(self, goal=None, repellers=None, funnels=None, hemispheres=None, attractors=None, first_arm=0):
        """The host form (vfik_move_scene_host): NumPy arrays of doubles, rounded to the engine's dtype exactly as ``set_fields``
        rounds the parameters.  Synchronous."""
        given = {"goal": goal, "repellers": repellers, "funnels": funnels, "hemispheres": hemispheres, "attractors": attractors}
        mv = _abi.SceneMove()
        keep, n_arms = [], None
        for name, member, cnt, tail in self._SCENE_ROWS:
            if given[name] is None:
                continue
            a = np.ascontiguousarray(given[name], dtype=np.float64)
            if cnt is None:
                ok = a.ndim >= 2 and a.size == a.shape[0] * tail
            else:
                ok = a.ndim >= 3 and a.size == a.shape[0] * a.shape[1] * tail
            if not ok:
                raise ValueError("%s must be (n_arms, %s%d), got %s" % (name, "" if cnt is None else "rows, ", tail, a.shape))
            if n_arms is not None and a.shape[0] != n_arms:
                raise ValueError("every array of a scene move must cover the same arms")
            n_arms = a.shape[0]
            keep.append(a)
            setattr(mv, member, a.ctypes.data)
            if cnt is not None:
                setattr(mv, cnt, a.shape[1])
        if n_arms is None:
            raise ValueError("give at least one of goal, repellers, funnels, hemispheres, attractors")
        self._chk(self.lib.vfik_move_scene_host(self.h, int(first_arm), n_arms, C.byref(mv)))

    def set_objects(self, frames, first_arm=0):
        """Object frames of the distance monitor (monitor_distance:72,111-129): (n_arms, n_objects, 16) doubles, kept on the
        device; a cycle call that asks for ``obj_dist`` then gets every arm's distance / angle to its objects."""
        f = np.ascontiguousarray(frames, dtype=np.float64)
        if f.ndim != 3 or f.shape[2] != 16:
            raise ValueError("frames must be (n_arms, n_objects, 16)")
        self._chk(self.lib.vfik_set_objects(self.h, int(first_arm), f.shape[0], f.ctypes.data, f.shape[1]))
        self.n_objects = f.shape[1]
        self._make_specs()

    def set_mixer_weights(self, weights, first_arm=0):
        """Per-arm mixer weights (n_arms, 6); ``None`` returns to the batch-wide ``params.mix_w``."""
        if weights is None:
            self._chk(self.lib.vfik_set_mixer_weights(self.h, 0, 0, None))
            return
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1, _abi.MIX_CHANNELS)
        self._chk(self.lib.vfik_set_mixer_weights(self.h, int(first_arm), w.shape[0], w.ctypes.data))

    def set_ext_cmd(self, channel, cmd):
        if cmd is None:
            self._chk(self.lib.vfik_set_ext_cmd(self.h, int(channel), None))
            return
        a = np.ascontiguousarray(cmd, dtype=self.io_dtype)
        if a.shape != (self.batch, self.n):
            raise ValueError("cmd must be (batch, n)")
        self._chk(self.lib.vfik_set_ext_cmd(self.h, int(channel), a.ctypes.data))

    def reset_state(self):
        self._chk(self.lib.vfik_reset_state(self.h))

    @property
    def slots_in_use(self):
        return self.lib.vfik_slots_in_use(self.h)

    @property
    def field_path(self):
        """0 general, 1 straight-line (goal + decay repellers of one integer order), 2 straight-line with an aux block (one funnel and / or one hemisphere per arm)."""
        return self.lib.vfik_field_path(self.h)

    @property
    def uniform_repellers(self):
        """True when every decay repeller of the batch shares one safe distance and one force (the uniform repeller image is read)."""
        return bool(self.lib.vfik_uniform_repellers(self.h))

    @property
    def one_chunk(self):
        """True when the lean float32 launches take the kernel's one-chunk order-5 body (include/vfik.h: vfik_one_chunk)."""
        return bool(self.lib.vfik_one_chunk(self.h))

    @property
    def dh_pattern(self):
        """1 when the chain matches a DH pattern the lean kernels are specialised for (include/vfik.h: vfik_dh_pattern), else 0."""
        return int(self.lib.vfik_dh_pattern(self.h))

    @property
    def launch_epoch(self):
        """Moves with every call that can change what a launch bakes in: a captured hipGraph of steps is valid for the epoch it was
        captured under (include/vfik.h: vfik_launch_epoch)."""
        return int(self.lib.vfik_launch_epoch(self.h))

    @property
    def mixed_orders(self):
        """True when the batch's decay repellers have integer orders that differ (the order planes are read; ABI 5)."""
        return bool(self.lib.vfik_mixed_orders(self.h))

    @property
    def device_bytes(self):
        return self.lib.vfik_device_bytes(self.h)

    # -- one control cycle -----------------------------------------------------------------------
    def _make_specs(self):
        """(shape, dtype) of the host array of every member of IO, inputs and outputs apart: a name of the one table is no key of the other.
        obj_dist [B][n_objects][2] -- one /dmonitor/distOut entry per object frame -- is in it once set_objects gave the count."""
        def rows(d):
            return (self.batch, self.n if d == "n" else d), self.io_dtype
        i32 = ((self.batch,), np.dtype(np.int32))
        self._in_specs = dict({k: rows(d) for k, d in _IN_SHAPES.items()}, active=i32)
        self._out_specs = dict({k: rows(d) for k, d in _OUT_SHAPES.items()}, status=i32)
        if self.n_objects >= 1:
            self._out_specs["obj_dist"] = ((self.batch, self.n_objects, 2), self.io_dtype)

    def _out_spec(self, key):
        if key == "obj_dist" and self.n_objects < 1:
            raise VfikError("obj_dist needs set_objects first")
        return self._out_specs[key]

    def _host_in(self, name, arr):
        """An input of a host-array call as the library reads it: contiguous, of the member's dtype (active: 0 / 1), shape checked."""
        shape, dtype = self._in_specs[name]
        a = np.ascontiguousarray(np.asarray(arr) != 0 if name == "active" else arr, dtype=dtype)
        if a.shape != shape:
            raise ValueError("null_control must be (batch, 4)" if name == "null_control" else "%s must be %s, got %s" % (name, shape, a.shape))
        return a

    def _host_io(self, q, null_control=None, q_ref=None, q_cmded=None, active=None, q_lo=None, q_hi=None, want=(), into=None):
        """The IO block of a host-array call (step_host, rollout_host, goto_host).  Returns (io, out, keep): ``out`` the output arrays named
        in ``want`` -- those of ``into`` where it has them, zeros otherwise --, ``keep`` the converted inputs by name, which must stay
        alive until the call returns."""
        keep = {"q": self._host_in("q", q)}
        if (q_lo is None) != (q_hi is None):
            raise ValueError("q_lo and q_hi come together")
        for name, arr in (("active", active), ("q_lo", q_lo), ("q_hi", q_hi), ("q_ref", q_ref), ("q_cmded", q_cmded), ("null_control", null_control)):
            if arr is not None:
                keep[name] = self._host_in(name, arr)
        io, out = IO(), {}
        for name, a in keep.items():
            setattr(io, name, a.ctypes.data)
        for k in want:
            shape, dtype = self._out_spec(k)
            if into is not None and k in into:
                out[k] = into[k]
                self._check_host(k, out[k], shape, dtype)
            else:
                out[k] = np.zeros(shape, dtype=dtype)
            setattr(io, k, out[k].ctypes.data)
        return io, out, keep

    def step_host(self, q, null_control=None, want=("qdot_out",), q_ref=None, q_cmded=None, active=None, q_lo=None, q_hi=None,
                  into=None):
        """Host arrays in, host arrays out (copies + sync inside the library).  q_ref: /jpctrl/ref of the
        joint P controller (mixer channel 2); q_cmded: the LWR's commanded-position echo (bridge:199-203);
        active: fresh-q gate (B,) -- arms with 0 publish nothing and keep their state (vf:312-313); q_lo / q_hi:
        this cycle's joint limits per arm (nullspace:167).  `into`: a dict of arrays from an earlier call to write
        into (rows of gated arms then keep their previous content instead of zeros)."""
        io, out, keep = self._host_io(q, null_control, q_ref, q_cmded, active, q_lo, q_hi, want, into)
        self._chk(self.lib.vfik_step_host(self.h, C.byref(io)))
        return out

    # -- pipelined host path (vfik_submit_host / vfik_wait) ------------------------------------------
    def host_array(self, shape, dtype=None):
        """A pinned host array (hipHostMalloc) that submit_host can copy from / to asynchronously.
        Freed with the engine (close)."""
        dtype = np.dtype(self.io_dtype if dtype is None else dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = self.lib.vfik_host_alloc(self.h, max(nbytes, 1))
        if not p:
            raise VfikError("vfik_host_alloc: " + self.lib.vfik_last_error().decode())
        self._pinned.append(p)
        buf = (C.c_char * max(nbytes, 1)).from_address(p)
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def submit_host(self, q, outs, null_control=None, q_ref=None, q_cmded=None, active=None, q_lo=None, q_hi=None):
        """Asynchronous vfik_step_host: ``q`` and the arrays of ``outs`` ({"qdot_out": array, ...}) must
        be C-contiguous arrays of the engine's dtype (``status`` and ``active``: int32) that stay untouched until
        :meth:`wait` -- use :meth:`host_array` (pinned memory) for overlap: copies from / to pageable memory make the
        call synchronous.  Returns the ticket."""
        io = IO()
        # (the caller's arrays as they are: checked, never converted)
        given = [("q", q), ("null_control", null_control), ("q_ref", q_ref), ("q_cmded", q_cmded), ("q_lo", q_lo), ("q_hi", q_hi)]
        for name, arr in [(k, a) for k, a in given if a is not None]:
            self._check_host(name, arr, *self._in_specs[name])
            setattr(io, name, arr.ctypes.data)
        if (q_lo is None) != (q_hi is None):
            raise ValueError("q_lo and q_hi come together")
        if active is not None:
            self._check_host("active", active, *self._in_specs["active"])
            io.active = active.ctypes.data
        for k, arr in outs.items():
            self._check_host(k, arr, *self._out_spec(k))
            setattr(io, k, arr.ctypes.data)
        t = C.c_long(-1)
        self._chk(self.lib.vfik_submit_host(self.h, C.byref(io), C.byref(t)))
        return int(t.value)

    @staticmethod
    def _check_host(name, arr, shape, dtype):
        if not isinstance(arr, np.ndarray) or arr.shape != tuple(shape) or arr.dtype != np.dtype(dtype) or not arr.flags.c_contiguous:
            raise ValueError("%s must be a C-contiguous %s array of shape %s" % (name, np.dtype(dtype).name, tuple(shape)))

    def wait(self, ticket):
        self._chk(self.lib.vfik_wait(self.h, int(ticket)))

    def rollout_host(self, q, n_cycles, dt, null_control=None, clamp=False, want=("qdot_out",), q_ref=None, active=None, q_lo=None,
                     q_hi=None, into=None):
        """n_cycles control cycles in one launch with q integrated on the device.
        Returns the outputs of the last cycle plus ``q`` = joint angles after it.  Arms gated off by ``active`` store
        nothing: their row of ``q`` comes back as it went in (a silent arm keeps its joint angles -- feeding the result into
        the next rollout is the normal closed-loop use), and their rows of the other outputs keep what ``into`` (a dict of
        arrays from an earlier call, as in :meth:`step_host`) held, zeros without it."""
        io, out, keep = self._host_io(q, null_control, q_ref, None, active, q_lo, q_hi, want, into)
        out["q"] = keep["q"].copy()  # gated arms keep their angles (the kernel stores nothing for them)
        self._chk(self.lib.vfik_rollout_host(self.h, C.byref(io), int(n_cycles), float(dt), 1 if clamp else 0, out["q"].ctypes.data))
        return out

    def rollout(self, io, n_cycles, dt, q_out=None, clamp=False):
        """Asynchronous device-pointer form of :meth:`rollout_host`."""
        self._chk(self.lib.vfik_rollout(self.h, C.byref(io), int(n_cycles), float(dt), 1 if clamp else 0, C.c_void_p(_ptr(q_out))))

    # -- timed moves: batched goto, waypoint lists and their joint-space forms (vfik_goto, vfik_follow, vfik_goto_js, vfik_follow_js:
    #    handlers.py:346-440 and set_ref_js, handlers.py:544-576, for the batch) --------------------------------------------------
    @staticmethod
    def _move_opts(cls, n_cycles, dt, stride, hold, clamp):
        o = cls()
        o.n_cycles, o.stride, o.dt = int(n_cycles), int(stride), float(dt)
        o.clamp_to_limits, o.hold = (1 if clamp else 0), (1 if hold else 0)
        return o

    def _check_dev(self, specs):
        """Contiguity, dtype and shape of the device arrays of a goto / follow call: (name, array, shape or None, dtype name) each."""
        for name, x, shape, dt_name in specs:
            if x is None or isinstance(x, int):
                continue
            if not x.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
            if str(x.dtype).split(".")[-1] != dt_name or (shape is not None and tuple(x.shape) != shape):
                raise ValueError("%s must be %s of shape %s, got %s %s" % (name, dt_name, shape, x.dtype, tuple(x.shape)))

    def _dev_specs(self, o, **arrays):
        """:meth:`_check_dev`'s specs of the options' arrays by their names, for the device forms."""
        B, n, ft, n_checks = self.batch, self.n, self.io_dtype.name, o.n_cycles // max(o.stride, 1)
        shapes = {"arrived": ((B,), "int32"), "reached": ((B, getattr(o, "n_way", 0)), "int32"), "next": ((B,), "int32"),
                  "pending": ((n_checks,), "int32"), "q_out": ((B, n), ft), "diff": ((B, n), ft), "q_traj": ((n_checks, B, n), ft),
                  "dist_traj": ((n_checks, B, 2), ft), "way_traj": ((n_checks, B), "int32"), "way": (None, ft), "wayq": (None, ft),
                  "kind": ((B, getattr(o, "n_way", 0)), "int32")}
        return tuple((k, x) + shapes[k] for k, x in arrays.items())

    @staticmethod
    def _list_len(name, x, well_formed, form, items, n_way):
        """n_way of a device form's list argument (way or wayq): a tensor's own, which an n_way beside it must agree with; a raw address
        needs n_way."""
        if isinstance(x, int):
            if n_way is None:
                raise ValueError("a raw %s address needs n_way" % name)
            return n_way
        if not well_formed(x):
            raise ValueError("%s must be %s, got %s" % (name, form, tuple(x.shape)))
        if n_way is not None and n_way != x.shape[1]:
            raise ValueError("%s: %d %s per arm, n_way says %d" % (name, x.shape[1], items, n_way))
        return x.shape[1]

    def _move_host(self, fn, io, o, out, keep, poll, arrays, traces):
        """The tail of the host forms: ``q``, the options' ``arrays`` and ``traces`` (by name) allocated with their fill values and wired
        into ``o``, the call, ``checks_run``, and ``pending`` and the traces cut to the checks that ran."""
        B, n, ft, n_checks = self.batch, self.n, self.io_dtype, max(o.n_cycles // max(o.stride, 1), 0)
        kinds = {"arrived": ((B,), np.int32, -1), "reached": ((B, getattr(o, "n_way", 0)), np.int32, -1), "next": ((B,), np.int32, 0),
                 "pending": ((n_checks,), np.int32, 0), "diff": ((B, n), ft, 0), "q_traj": ((n_checks, B, n), ft, 0),
                 "dist_traj": ((n_checks, B, 2), ft, 0), "way_traj": ((n_checks, B), np.int32, -1)}
        out["q"] = keep["q"].copy()
        o.q_out = out["q"].ctypes.data
        for k in arrays + traces:
            shape, dtype, fill = kinds[k]
            out[k] = np.full(shape, fill, dtype=dtype)
            setattr(o, k, out[k].ctypes.data)
        ran = C.c_int(0)
        self._chk(fn(self.h, C.byref(io), C.byref(o), int(poll), C.byref(ran)))
        out["checks_run"] = int(ran.value)
        if self._stall_rule is not None:
            out["stalled"] = self.stalled()
        if self._wait_rule is not None:
            out["waited"] = self.waited()
        for k in ("pending",) + traces:
            out[k] = out[k][:out["checks_run"]]
        return out

    def set_stall_rule(self, patience, eps=(0.0, 0.0), eps_js=0.0, stop=True, stalled=None):
        """Declare arms that make no progress stalled, on the device, in every timed move from now on (include/vfik.h:
        vfik_set_stall_rule); ``patience=None`` switches the rule off again, the default.  An arm under way whose measure -- distance and
        angle to its goal, or the largest joint error -- has not improved on its best by more than ``eps`` = (metres, radians) or
        ``eps_js`` for ``patience`` checks in a row is stalled: no rule is applied to it again, it leaves ``pending`` (so ``poll`` ends a
        host form without it) and, with ``stop``, it takes no further cycle.  ``stalled``: an int32 (batch,) torch tensor on this device
        or a raw device address that receives every arm's stall cycle (-1: not stalled), else the engine keeps its own (:meth:`stalled`).
        While a rule is set every ``*_host`` form returns a ``"stalled"`` key."""
        if patience is None:
            self._chk(self.lib.vfik_set_stall_rule(self.h, None))
            self._stall_rule = None
            return
        self._check_dev((("stalled", stalled, (self.batch,), "int32"),))
        r = _abi.StallRule()
        r.patience, r.stop = int(patience), (1 if stop else 0)
        r.eps_pos, r.eps_rot = map(float, eps)
        r.eps_js = float(eps_js)
        r.stalled = _ptr(stalled)
        self._chk(self.lib.vfik_set_stall_rule(self.h, C.byref(r)))
        self._stall_rule = (r, stalled)

    def stalled(self):
        """int32 (batch,): the cycle index of the check that declared each arm stalled in the last timed move, -1 for an arm that
        did not stall (vfik_stalled_host; synchronises).  Needs a stall rule."""
        out = np.empty(self.batch, dtype=np.int32)
        self._chk(self.lib.vfik_stalled_host(self.h, C.c_void_p(out.ctypes.data)))
        return out

    def _js_precision(self, precision, name="precision"):
        """goal_precision per joint as the library reads it: float64 (n,), each >= 0 and not NaN."""
        p = np.ascontiguousarray(precision, dtype=np.float64)
        if p.shape != (self.n,):
            raise ValueError("%s must be a sequence of %d values (one per joint), got shape %s" % (name, self.n, p.shape))
        return p

    def goto(self, io, n_cycles, dt, precision, stride=1, hold=False, clamp=False, arrived=None, pending=None, q_out=None, q_traj=None,
             dist_traj=None):
        """Drive the arms to their goals and report arrival, asynchronously on the engine's stream (include/vfik.h: vfik_goto):
        ``n_cycles / stride`` blocks of ``stride`` control cycles from ``io.q`` (``io`` from :meth:`make_io`), after each block one
        arrival check against ``precision`` = (metres, radians) -- gotoFrame's goal_precision.  ``arrived``: int32 (B,), required, the
        cycle index of each arm's first successful check or -1; ``pending``: int32 (n_checks,), arms still under way after every check;
        ``q_out`` (B, n); ``q_traj`` (n_checks, B, n); ``dist_traj`` (n_checks, B, 2).  Torch tensors on this device or raw addresses.
        ``hold``: an arm that arrived takes no further cycle."""
        if arrived is None:
            raise ValueError("goto needs arrived, an int32 (batch,) device array")
        o = self._move_opts(_abi.GotoOpts, n_cycles, dt, stride, hold, clamp)
        self._check_dev(self._dev_specs(o, arrived=arrived, pending=pending, q_out=q_out, q_traj=q_traj, dist_traj=dist_traj))
        o.pos_prec, o.rot_prec = map(float, precision)
        o.arrived, o.pending, o.q_out, o.q_traj, o.dist_traj = _ptr(arrived), _ptr(pending), _ptr(q_out), _ptr(q_traj), _ptr(dist_traj)
        self._chk(self.lib.vfik_goto(self.h, C.byref(io), C.byref(o)))

    def goto_host(self, q, n_cycles, dt, precision, stride=1, hold=False, clamp=False, trajectory=False, poll=0, want=("qdot_out",),
                  null_control=None, active=None, q_lo=None, q_hi=None, q_ref=None):
        """Host arrays in, host arrays out (vfik_goto_host; synchronous).  Returns a dict with ``q`` (joint angles after the last block
        executed; held arms: at arrival), ``arrived`` (B,), ``pending`` (checks_run,), ``checks_run``, the rows named in ``want`` (every
        arm's: those of its last evaluated cycle) and, with ``trajectory``, ``q_traj`` (checks_run, B, n) and ``dist_traj``
        (checks_run, B, 2).  ``poll`` > 0: after every ``poll`` checks the count of arms still under way is read back and the goto ends
        once it is 0 -- ``checks_run`` then tells how far it went.  Arms gated off by ``active`` never run and never arrive."""
        io, out, keep = self._host_io(q, null_control, q_ref, None, active, q_lo, q_hi, want)
        o = self._move_opts(_abi.GotoOpts, n_cycles, dt, stride, hold, clamp)
        o.pos_prec, o.rot_prec = map(float, precision)
        return self._move_host(self.lib.vfik_goto_host, io, o, out, keep, poll, ("arrived", "pending"),
                               ("q_traj", "dist_traj") if trajectory else ())

    @staticmethod
    def _follow_precision(o, precision, via_precision):
        o.pos_prec, o.rot_prec = map(float, precision)
        o.via_pos_prec, o.via_rot_prec = map(float, precision if via_precision is None else via_precision)

    def follow(self, io, way, n_cycles, dt, precision, via_precision=None, stride=1, hold=False, clamp=False, reached=None, next=None,
               pending=None, q_out=None, q_traj=None, dist_traj=None, way_traj=None, n_way=None):
        """Drive every arm along its own list of goal frames, asynchronously on the engine's stream (include/vfik.h: vfik_follow):
        :meth:`goto`'s blocks and checks, and the check that finds an arm at waypoint w puts waypoint w + 1 into the arm's goal block on
        the device.  ``way``: (B, W, 16) or (B, W, 4, 4) row-major frames of the engine's dtype, 16-byte aligned; a row whose first
        element is NaN ends the arm's path (no row: the arm is kept out like one gated off by ``io.active``).  ``precision`` =
        (metres, radians) holds at an arm's last waypoint, ``via_precision`` at those before it (None: ``precision``).  ``reached``:
        int32 (B, W), required, the cycle index of the check that found the arm at each waypoint or -1; ``next``: int32 (B,), required,
        the number of waypoints reached; ``pending``: int32 (n_checks,); ``q_out``, ``q_traj``, ``dist_traj`` as :meth:`goto`;
        ``way_traj``: int32 (n_checks, B), the waypoint each row of ``dist_traj`` was measured against.  Torch tensors on this device, or
        raw addresses (``way`` then with ``n_way``).  ``hold``: an arm that reached its last waypoint takes no further cycle.
        Afterwards the goal block of an arm holds the waypoint it was last sent to.  The Python-side ``FieldSets`` mirror of the host
        layer does not learn of it, as with :meth:`move_fields`: a later ``set_fields`` from the mirror puts the old goal back."""
        if reached is None or next is None:
            raise ValueError("follow needs reached, an int32 (batch, n_way) device array, and next, an int32 (batch,) one")
        n_way = self._list_len("way", way, lambda w: w.dim() in (3, 4) and w.shape[0] == self.batch and w.numel() == self.batch * w.shape[1] * 16,
                               "(batch, n_way, 16) or (batch, n_way, 4, 4)", "waypoints", n_way)
        o = self._move_opts(_abi.FollowOpts, n_cycles, dt, stride, hold, clamp)
        o.n_way = int(n_way)
        self._check_dev(self._dev_specs(o, way=way, reached=reached, next=next, pending=pending, q_out=q_out, q_traj=q_traj,
                                        dist_traj=dist_traj, way_traj=way_traj))
        self._follow_precision(o, precision, via_precision)
        o.way16, o.reached, o.next, o.pending = _ptr(way), _ptr(reached), _ptr(next), _ptr(pending)
        o.q_out, o.q_traj, o.dist_traj, o.way_traj = _ptr(q_out), _ptr(q_traj), _ptr(dist_traj), _ptr(way_traj)
        self._chk(self.lib.vfik_follow(self.h, C.byref(io), C.byref(o)))

    def follow_host(self, q, way, n_cycles, dt, precision, via_precision=None, stride=1, hold=False, clamp=False, trajectory=False, poll=0,
                    want=("qdot_out",), null_control=None, active=None, q_lo=None, q_hi=None, q_ref=None):
        """Host arrays in, host arrays out (vfik_follow_host; synchronous).  ``way``: (B, W, 16) or (B, W, 4, 4), converted to the
        engine's dtype; NaN rows end a path.  Returns what :meth:`goto_host` returns without ``arrived``, plus ``reached`` (B, W),
        ``next`` (B,) and, with ``trajectory``, ``way_traj`` (checks_run, B).  ``poll`` > 0 ends the call once every arm that takes part
        is at its last waypoint.  The ``FieldSets`` mirror does not learn of the new goals (see :meth:`follow`)."""
        w = np.asarray(way)
        if w.ndim not in (3, 4) or w.shape[0] != self.batch or w.size != self.batch * w.shape[1] * 16 or w.shape[1] < 1:
            raise ValueError("way must be (batch, n_way, 16) or (batch, n_way, 4, 4), got %s" % (w.shape,))
        w = np.ascontiguousarray(w, dtype=self.io_dtype).reshape(self.batch, w.shape[1], 16)
        if w.ctypes.data % 16:   # (NumPy aligns to 16 bytes or more where it allocates; a view of the caller's may not be)
            buf = np.empty(w.size + 4, dtype=self.io_dtype)
            off = (-buf.ctypes.data % 16) // buf.itemsize
            buf = buf[off:off + w.size].reshape(w.shape)
            buf[...] = w
            w = buf
        io, out, keep = self._host_io(q, null_control, q_ref, None, active, q_lo, q_hi, want)
        o = self._move_opts(_abi.FollowOpts, n_cycles, dt, stride, hold, clamp)
        self._follow_precision(o, precision, via_precision)
        o.n_way, o.way16 = w.shape[1], w.ctypes.data
        return self._move_host(self.lib.vfik_follow_host, io, o, out, keep, poll, ("reached", "next", "pending"),
                               ("q_traj", "dist_traj", "way_traj") if trajectory else ())

    def goto_js(self, io, n_cycles, dt, precision, stride=1, hold=False, clamp=False, arrived=None, pending=None, q_out=None, q_traj=None,
                diff=None):
        """Drive the arms to the joint references ``io.q_ref`` and report arrival, asynchronously on the engine's stream (include/vfik.h:
        vfik_goto_js): :meth:`goto`'s blocks, and after each one set_ref_js's rule ``(ref - precision <= q) & (ref + precision >= q)`` on
        every joint.  ``precision``: a length-n sequence (host values), goal_precision per joint.  ``arrived``: int32 (B,), required;
        ``pending``: int32 (n_checks,); ``q_out``, ``diff`` (B, n) -- ``ref - q`` of each arm's last check; ``q_traj`` (n_checks, B, n).  Torch
        tensors on this device or raw addresses.  The mixer flag and weights are the caller's (joint control: ``mix_w = [0, 0, 1, 0, 0, 0]``
        with ``F_MIXER``)."""
        if arrived is None:
            raise ValueError("goto_js needs arrived, an int32 (batch,) device array")
        o = self._move_opts(_abi.GotoJsOpts, n_cycles, dt, stride, hold, clamp)
        self._check_dev(self._dev_specs(o, arrived=arrived, pending=pending, q_out=q_out, q_traj=q_traj, diff=diff))
        prec = self._js_precision(precision)
        o.prec = prec.ctypes.data
        o.arrived, o.pending, o.q_out, o.q_traj, o.diff = _ptr(arrived), _ptr(pending), _ptr(q_out), _ptr(q_traj), _ptr(diff)
        self._chk(self.lib.vfik_goto_js(self.h, C.byref(io), C.byref(o)))

    def goto_js_host(self, q, q_ref, n_cycles, dt, precision, stride=1, hold=False, clamp=False, trajectory=False, poll=0, want=("qdot_out",),
                     null_control=None, active=None, q_lo=None, q_hi=None):
        """Host arrays in, host arrays out (vfik_goto_js_host; synchronous).  Returns what :meth:`goto_host` returns, with ``diff`` (B, n)
        -- ``q_ref - q`` of every arm's last check, set_ref_js's ``difference`` -- and without ``dist_traj``: ``q``, ``arrived``, ``pending``,
        ``checks_run``, the rows named in ``want`` and, with ``trajectory``, ``q_traj`` (checks_run, B, n).  A row of ``q_ref`` that starts
        with NaN is an arm without a joint controller: it runs and never arrives."""
        if q_ref is None:
            raise ValueError("goto_js_host needs q_ref, the joint reference of every arm")
        io, out, keep = self._host_io(q, null_control, q_ref, None, active, q_lo, q_hi, want)
        prec = self._js_precision(precision)
        o = self._move_opts(_abi.GotoJsOpts, n_cycles, dt, stride, hold, clamp)
        o.prec = prec.ctypes.data
        return self._move_host(self.lib.vfik_goto_js_host, io, o, out, keep, poll, ("arrived", "pending", "diff"),
                               ("q_traj",) if trajectory else ())

    def _follow_js_precision(self, o, precision, via_precision):
        """The two precision arrays into the options; returned because the options hold their addresses only (the caller keeps them until
        the call is over)."""
        prec = self._js_precision(precision)
        via = None if via_precision is None else self._js_precision(via_precision, "via_precision")
        o.prec, o.via_prec = prec.ctypes.data, (None if via is None else via.ctypes.data)
        return prec, via

    def follow_js(self, io, wayq, n_cycles, dt, precision, via_precision=None, stride=1, hold=False, clamp=False, reached=None, next=None,
                  pending=None, q_out=None, q_traj=None, diff=None, way_traj=None, n_way=None):
        """Drive every arm along its own list of postures, asynchronously on the engine's stream (include/vfik.h: vfik_follow_js):
        :meth:`follow`'s state machine with :meth:`goto_js`'s rule.  ``wayq``: (B, W, n) of the engine's dtype; a row whose first element
        is NaN ends the arm's list.  ``io.q_ref`` must be left out: the reference row belongs to the engine.  ``precision`` (length n) holds
        at an arm's last posture, ``via_precision`` at those before it (None: ``precision``).  ``reached`` int32 (B, W) and ``next`` int32
        (B,) are required; ``pending``, ``q_out``, ``q_traj``, ``diff`` as :meth:`goto_js`; ``way_traj``: int32 (n_checks, B).  Torch tensors
        on this device, or raw addresses (``wayq`` then with ``n_way``)."""
        if reached is None or next is None:
            raise ValueError("follow_js needs reached, an int32 (batch, n_way) device array, and next, an int32 (batch,) one")
        n_way = self._list_len("wayq", wayq, lambda w: w.dim() == 3 and w.shape[0] == self.batch and w.shape[2] == self.n,
                               "(batch, n_way, %d)" % self.n, "postures", n_way)
        o = self._move_opts(_abi.FollowJsOpts, n_cycles, dt, stride, hold, clamp)
        o.n_way = int(n_way)
        self._check_dev(self._dev_specs(o, wayq=wayq, reached=reached, next=next, pending=pending, q_out=q_out, q_traj=q_traj, diff=diff,
                                        way_traj=way_traj))
        kept = self._follow_js_precision(o, precision, via_precision)  # noqa: F841
        o.wayq, o.reached, o.next, o.pending = _ptr(wayq), _ptr(reached), _ptr(next), _ptr(pending)
        o.q_out, o.q_traj, o.diff, o.way_traj = _ptr(q_out), _ptr(q_traj), _ptr(diff), _ptr(way_traj)
        self._chk(self.lib.vfik_follow_js(self.h, C.byref(io), C.byref(o)))

    def follow_js_host(self, q, wayq, n_cycles, dt, precision, via_precision=None, stride=1, hold=False, clamp=False, trajectory=False,
                       poll=0, want=("qdot_out",), null_control=None, active=None, q_lo=None, q_hi=None):
        """Host arrays in, host arrays out (vfik_follow_js_host; synchronous).  ``wayq``: (B, W, n), converted to the engine's dtype; a row
        that starts with NaN ends a list.  Returns what :meth:`goto_js_host` returns without ``arrived``, plus ``reached`` (B, W), ``next``
        (B,) and, with ``trajectory``, ``way_traj`` (checks_run, B).  ``poll`` > 0 ends the call once every arm that takes part is at its
        last posture."""
        w = np.asarray(wayq)
        if w.ndim != 3 or w.shape[0] != self.batch or w.shape[1] < 1 or w.shape[2] != self.n:
            raise ValueError("wayq must be (batch, n_way, %d), got %s" % (self.n, w.shape))
        w = np.ascontiguousarray(w, dtype=self.io_dtype)
        io, out, keep = self._host_io(q, null_control, None, None, active, q_lo, q_hi, want)
        o = self._move_opts(_abi.FollowJsOpts, n_cycles, dt, stride, hold, clamp)
        kept = self._follow_js_precision(o, precision, via_precision)  # noqa: F841
        o.n_way, o.wayq = w.shape[1], w.ctypes.data
        return self._move_host(self.lib.vfik_follow_js_host, io, o, out, keep, poll, ("reached", "next", "pending", "diff"),
                               ("q_traj", "way_traj") if trajectory else ())

    # -- motion scripts: frames and postures in one list per arm (vfik_script) ------------------------------------------------------
    def _script_opts(self, n_cycles, dt, stride, hold, clamp, precision, via_precision, js_precision, js_via_precision, mix_frame,
                     mix_posture):
        """The options of a script without its arrays, and the precision arrays they point into (the caller keeps them until the call
        is over)."""
        o = self._move_opts(_abi.ScriptOpts, n_cycles, dt, stride, hold, clamp)
        self._follow_precision(o, precision, via_precision)
        prec = self._js_precision(js_precision, "js_precision")
        via = None if js_via_precision is None else self._js_precision(js_via_precision, "js_via_precision")
        o.prec, o.via_prec = prec.ctypes.data, (None if via is None else via.ctypes.data)
        for name, dst, src in (("mix_frame", o.mix_frame, mix_frame), ("mix_posture", o.mix_posture, mix_posture)):
            w = np.asarray(src, dtype=np.float64)
            if w.shape != (4,):
                raise ValueError("%s must be 4 mixer weights (channels 0..3), got shape %s" % (name, w.shape))
            for i in range(4):
                dst[i] = float(w[i])
        return o, (prec, via)

    def script(self, io, kind, way, wayq, n_cycles, dt, precision, js_precision, via_precision=None, js_via_precision=None,
               mix_frame=_abi.MIX_FRAME, mix_posture=_abi.MIX_POSTURE, stride=1, hold=False, clamp=False, reached=None, next=None,
               pending=None, q_out=None, q_traj=None, dist_traj=None, diff=None, way_traj=None, n_way=None):
        """Run every arm's own motion script, asynchronously on the engine's stream (include/vfik.h: vfik_script): :meth:`follow`'s
        state machine over a list whose steps are goal frames or postures.  ``kind``: int32 (B, W), ``_abi.STEP_FRAME`` or
        ``_abi.STEP_POSTURE``, any other value ends the arm's script (an arm without a step is kept out); ``way``: (B, W, 16) or
        (B, W, 4, 4), 16-byte aligned, read at frame steps; ``wayq``: (B, W, n), read at posture steps.  ``precision`` / ``via_precision``
        = (metres, radians) as :meth:`follow`, ``js_precision`` / ``js_via_precision`` (length n) as :meth:`follow_js`.  ``mix_frame`` and
        ``mix_posture``: the mixer weights of channels 0..3 an arm runs under on its way to a frame or to a posture -- by default what the
        reference's cartesian_controller() and joint_controller() send.  ``io.q_ref`` must be left out.  ``reached`` int32 (B, W) and
        ``next`` int32 (B,) are required; ``pending``, ``q_out``, ``q_traj``, ``dist_traj``, ``diff``, ``way_traj`` as :meth:`follow` and
        :meth:`follow_js`.  Torch tensors on this device, or raw addresses (then with ``n_way``).  The engine needs ``F_MIXER``; its own
        mixer weights and limiter speeds are read, never written."""
        if reached is None or next is None:
            raise ValueError("script needs reached, an int32 (batch, n_way) device array, and next, an int32 (batch,) one")
        n_way = self._list_len("way", way, lambda w: w.dim() in (3, 4) and w.shape[0] == self.batch and w.numel() == self.batch * w.shape[1] * 16,
                               "(batch, n_way, 16) or (batch, n_way, 4, 4)", "steps", n_way)
        n_way = self._list_len("wayq", wayq, lambda w: w.dim() == 3 and w.shape[0] == self.batch and w.shape[2] == self.n,
                               "(batch, n_way, %d)" % self.n, "steps", n_way)
        o, kept = self._script_opts(n_cycles, dt, stride, hold, clamp, precision, via_precision, js_precision, js_via_precision,  # noqa: F841
                                    mix_frame, mix_posture)
        o.n_way = int(n_way)
        self._check_dev(self._dev_specs(o, kind=kind, way=way, wayq=wayq, reached=reached, next=next, pending=pending, q_out=q_out,
                                        q_traj=q_traj, dist_traj=dist_traj, diff=diff, way_traj=way_traj))
        o.kind, o.way16, o.wayq, o.reached, o.next, o.pending = _ptr(kind), _ptr(way), _ptr(wayq), _ptr(reached), _ptr(next), _ptr(pending)
        o.q_out, o.q_traj, o.dist_traj, o.diff, o.way_traj = _ptr(q_out), _ptr(q_traj), _ptr(dist_traj), _ptr(diff), _ptr(way_traj)
        self._chk(self.lib.vfik_script(self.h, C.byref(io), C.byref(o)))

    def script_host(self, q, kind, way, wayq, n_cycles, dt, precision, js_precision, via_precision=None, js_via_precision=None,
                    mix_frame=_abi.MIX_FRAME, mix_posture=_abi.MIX_POSTURE, stride=1, hold=False, clamp=False, trajectory=False, poll=0,
                    want=("qdot_out",), null_control=None, active=None, q_lo=None, q_hi=None):
        """Host arrays in, host arrays out (vfik_script_host; synchronous).  ``kind`` (B, W), ``way`` (B, W, 16) or (B, W, 4, 4) and
        ``wayq`` (B, W, n) as :meth:`script`, converted to int32 and the engine's dtype.  Returns what :meth:`follow_host` returns plus
        ``diff`` (B, n): ``q``, ``reached`` (B, W), ``next`` (B,), ``pending``, ``checks_run``, the rows named in ``want`` and, with
        ``trajectory``, ``q_traj``, ``dist_traj`` and ``way_traj``.  ``poll`` > 0 ends the call once every arm that takes part is at
        its last step."""
        kd = np.ascontiguousarray(kind, dtype=np.int32)
        if kd.ndim != 2 or kd.shape[0] != self.batch or kd.shape[1] < 1:
            raise ValueError("kind must be (batch, n_way), got %s" % (kd.shape,))
        W = kd.shape[1]
        w = np.asarray(way)
        if w.ndim not in (3, 4) or w.shape[0] != self.batch or w.shape[1] != W or w.size != self.batch * W * 16:
            raise ValueError("way must be (batch, %d, 16) or (batch, %d, 4, 4), got %s" % (W, W, w.shape))
        w = np.ascontiguousarray(w, dtype=self.io_dtype).reshape(self.batch, W, 16)
        if w.ctypes.data % 16:   # (as follow_host)
            buf = np.empty(w.size + 4, dtype=self.io_dtype)
            off = (-buf.ctypes.data % 16) // buf.itemsize
            buf = buf[off:off + w.size].reshape(w.shape)
            buf[...] = w
            w = buf
        wq = np.asarray(wayq)
        if wq.shape != (self.batch, W, self.n):
            raise ValueError("wayq must be (batch, %d, %d), got %s" % (W, self.n, wq.shape))
        wq = np.ascontiguousarray(wq, dtype=self.io_dtype)
        io, out, keep = self._host_io(q, null_control, None, None, active, q_lo, q_hi, want)
        o, kept = self._script_opts(n_cycles, dt, stride, hold, clamp, precision, via_precision, js_precision, js_via_precision,  # noqa: F841
                                    mix_frame, mix_posture)
        o.n_way, o.kind, o.way16, o.wayq = W, kd.ctypes.data, w.ctypes.data, wq.ctypes.data
        return self._move_host(self.lib.vfik_script_host, io, o, out, keep, poll, ("reached", "next", "pending", "diff"),
                               ("q_traj", "dist_traj", "way_traj") if trajectory else ())

    def make_io(self, q, null_control=None, q_ref=None, q_cmded=None, active=None, q_lo=None, q_hi=None, **outs):
        """IO block from device pointers (torch tensors on this device, or raw addresses).  active: int32 [B]."""
        io = IO()
        io.q = _ptr(q)
        io.null_control = _ptr(null_control)
        io.q_ref = _ptr(q_ref)
        io.q_cmded = _ptr(q_cmded)
        io.active = _ptr(active)
        io.q_lo = _ptr(q_lo)
        io.q_hi = _ptr(q_hi)
        for k, v in outs.items():
            setattr(io, k, _ptr(v))
        return io

    def step(self, io):
        """Asynchronous launch on the handle's stream; ``io`` from :meth:`make_io`."""
        self._chk(self.lib.vfik_step(self.h, C.byref(io)))

    def stepper(self, io):
        """The hot enqueue as a zero-argument callable: ``byref(io)``, the handle and the prototype are bound ONCE, the
        return code is checked inline.  ``io`` (and the buffers it names) must outlive the callable; changing a member of
        ``io`` afterwards is seen by the next call (the library reads the struct at every launch).  What bench.py's timed loop and any
        closed-loop driver at rate should call: at a 5-us launch period the Python-side cost of ``step`` is a third of the budget."""
        fn, h, ref, err = self.lib.vfik_step, self.h, C.byref(io), self._chk

        def step():
            rc = fn(h, ref)
            if rc:
                err(rc)
        step.io = io  # keeps the struct alive
        return step

    def sync(self):
        self._chk(self.lib.vfik_sync(self.h))

    def time_steps(self, io, warmup, steps):
        ms = C.c_float(0.0)
        self._chk(self.lib.vfik_time_steps(self.h, C.byref(io), int(warmup), int(steps), C.byref(ms)))
        return float(ms.value)

    # -- device memory without torch -------------------------------------------------------------
    def dev_alloc(self, nbytes):
        p = self.lib.vfik_dev_alloc(self.h, int(nbytes))
        if not p:
            raise VfikError("vfik_dev_alloc: " + self.lib.vfik_last_error().decode())
        return p

    def dev_free(self, p):
        self._chk(self.lib.vfik_dev_free(self.h, C.c_void_p(p)))

    def h2d(self, dst, arr):
        a = np.ascontiguousarray(arr)
        self._chk(self.lib.vfik_memcpy_h2d(self.h, C.c_void_p(dst), a.ctypes.data, a.nbytes))

    def d2h(self, arr, src):
        self._chk(self.lib.vfik_memcpy_d2h(self.h, arr.ctypes.data, C.c_void_p(src), arr.nbytes))

    def set_max_vel(self, values, first_arm=0):
        """Per-arm limiter speed (the /bridge/max_vel value each bridge keeps, bridge:612-623)."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        self._chk(self.lib.vfik_set_max_vel(self.h, int(first_arm), len(v), v.ctypes.data))

    def set_arm_weights(self, wy=None, wq=None, first_arm=0):
        """Per-arm IK weights (vf:295-309): wy (n_arms, 6) and/or wq (n_arms, n) starting at first_arm."""
        arrs = []
        for w, cols in ((wy, 6), (wq, self.n)):
            if w is None:
                arrs.append(None)
                continue
            a = np.ascontiguousarray(w, dtype=np.float64)
            if a.ndim != 2 or a.shape[1] != cols:
                raise ValueError("weights must be (n_arms, %d), got %s" % (cols, a.shape))
            arrs.append(a)
        counts = {a.shape[0] for a in arrs if a is not None}
        if len(counts) != 1:
            raise ValueError("wy and wq must cover the same arms")
        self._chk(self.lib.vfik_set_arm_weights(self.h, int(first_arm), counts.pop(),
                                                None if arrs[0] is None else arrs[0].ctypes.data,
                                                None if arrs[1] is None else arrs[1].ctypes.data))

    def set_small_batch_kernel(self, max_batch):
        """Lean launches of batches up to max_batch arms take the eight-lanes-per-arm kernel (0 = never)."""
        self._chk(self.lib.vfik_set_small_batch_kernel(self.h, int(max_batch)))

    @property
    def small_batch_launches(self):
        return int(self.lib.vfik_small_batch_launches(self.h))

    def launched_kernels(self):
        """The set of cycle-kernel instantiations launched since the last call, by demangled name without namespace and parameter list
        (include/vfik.h: vfik_launched_kernels); the record is cleared."""
        n = self.lib.vfik_launched_kernels(self.h, None, 0)
        self._chk(min(n, 0))
        buf = C.create_string_buffer(n + 1)
        self._chk(min(self.lib.vfik_launched_kernels(self.h, buf, n + 1), 0))
        return set(buf.value.decode().splitlines())

    def probe_field(self, pose_dev, v6_dev):
        """The field of every arm at a given pose (vf:469-503): device pose[B][16] -> v6[B][6]."""
        self._chk(self.lib.vfik_probe_field(self.h, C.c_void_p(_ptr(pose_dev)), C.c_void_p(_ptr(v6_dev))))

    def object_distances(self, pose_dev, frames_dev, max_objects, out_dev):
        """Distance monitor (monitor_distance:148-167) on device arrays: out[B][max_objects][2]."""
        self._chk(self.lib.vfik_object_distances(self.h, C.c_void_p(_ptr(pose_dev)), C.c_void_p(_ptr(frames_dev)), int(max_objects),
                                                 C.c_void_p(_ptr(out_dev))))

    def track_error(self, pose_dev, v6_dev, out_dev, active_dev=None):
        """One step of the tracking-error estimator (vf:349-428) on device arrays; active_dev: int32 [B] gate
        (arms with 0 append no frame, vf:312-313), or None."""
        self._chk(self.lib.vfik_track_error(self.h, C.c_void_p(_ptr(pose_dev)), C.c_void_p(_ptr(v6_dev)), C.c_void_p(_ptr(out_dev)),
                                            C.c_void_p(_ptr(active_dev))))

    def track_reset(self):
        self._chk(self.lib.vfik_track_reset(self.h))

    def mix(self, cmds_dev, weights, out_dev):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        self._chk(self.lib.vfik_mix(self.h, C.c_void_p(_ptr(cmds_dev)), w.ctypes.data, len(w), C.c_void_p(_ptr(out_dev))))
