"""The cycle-kernel instantiations linked into the built library (vfclik_amd/csrc/libvfik_hip.so), read from the library itself:
its device code objects are extracted with llvm-objdump --offloading and their kernel symbols listed demangled.  Each name is
written as vfik_kernel.h's cycle_kernel_name writes it -- namespace and parameter list stripped, " [heavy]" behind the long chains'
non-lean single-cycle variants, which are a code object of their own (-DVFIK_HEAVY_PART, csrc/Makefile) -- and its template
arguments are parsed by the kernels' own parameter names.

A helper of the suite, not a conftest.py: tests/test_kernel_variants.py checks the list on the CPU, tests/test_gpu_variants.py runs
every variant on the GPU."""
import collections
import functools
import glob
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vfclik_amd", "csrc")
LIB = os.path.join(CSRC, "libvfik_hip.so")
OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")

# template parameters in the order the kernels declare them (vfik_kernel.hip); RESERVED: the removed persistent launch's slot, false in every kernel
PARAMS = {
    "cycle_kernel_s": ("T", "NJ", "NS", "PL", "ROLL", "FASTF", "LEAN", "CF", "RESERVED", "FUN", "WAVES", "UNI", "D"),
    "cycle_kernel_x": ("T", "NJ", "NS", "PL", "ROLL", "FASTF", "LEAN", "CF", "RESERVED", "FUN", "WAVES", "UNI", "MIXO", "D"),
    "cycle_kernel_m": ("T", "NJ", "NS", "LEAN", "FUN", "D"),
    "cycle_sub8_kernel": ("T", "NJ", "NS", "D"),
    "cycle_sub8_kernel_x": ("T", "NJ", "NS", "D"),
}
_SYM = re.compile(r"\bvfik::\(anonymous namespace\)::(cycle_\w+<[^<>]*>)\(")
HEAVY = " [heavy]"

Variant = collections.namedtuple("Variant", "name kernel args heavy")


def chain10(robots, Chain):
    """The 10-joint chain of the suite: the LWR's DH table and three more links, off every DH pattern (none is built for 10 joints)."""
    import math

    import numpy as np
    dh = list(robots._LWR_DH) + [(0.05, math.pi / 2, 0.1, 0.0), (0.0, -math.pi / 2, 0.12, 0.3), (0.08, 0.4, 0.0, 0.0)]
    lim = np.concatenate([robots._LWR_LIM, np.array([150, 120, 150]) * math.pi / 180])
    return Chain.from_dh(dh, -lim, lim, name="rand10")


def parse(name):
    """cycle_kernel_name's string -> Variant(name, kernel, args, heavy); args maps the template parameter names to int / bool / 'float' | 'double'."""
    heavy = name.endswith(HEAVY)
    m = re.fullmatch(r"(cycle_\w+)<([^<>]*)>", name[: -len(HEAVY)] if heavy else name)
    if not m or m.group(1) not in PARAMS:
        raise ValueError("not a cycle-kernel name: %r" % name)
    vals = [v.strip() for v in m.group(2).split(",")]
    keys = PARAMS[m.group(1)]
    if len(vals) != len(keys):
        raise ValueError("%r: %d template arguments, %s declares %d" % (name, len(vals), m.group(1), len(keys)))
    args = {}
    for k, v in zip(keys, vals):
        if k == "T":
            if v not in ("float", "double"):
                raise ValueError("%r: I/O type %r" % (name, v))
            args[k] = v
        elif v in ("true", "false"):
            args[k] = v == "true"
        else:
            args[k] = int(v)
    return Variant(name, m.group(1), args, heavy)


def group_of(v):
    """(joint count, I/O bits, nullspace module): the objects the library is compiled in."""
    return v.args["NJ"], 32 if v.args["T"] == "float" else 64, v.args["NS"]


def _code_objects(lib):
    """[[demangled symbol, ...] per device code object of the library]"""
    with tempfile.TemporaryDirectory() as d:
        link = os.path.join(d, "lib.so")
        os.symlink(os.path.abspath(lib), link)
        subprocess.run([OBJDUMP, "--offloading", link], cwd=d, check=True, capture_output=True, timeout=120)
        objs = []
        for f in sorted(glob.glob(os.path.join(d, "lib.so.*amdgcn*"))):
            out = subprocess.run([OBJDUMP, "--syms", "--demangle", f], check=True, capture_output=True, text=True, timeout=120).stdout
            objs.append([ln for ln in out.splitlines() if " F .text" in ln])
        return objs


@functools.lru_cache(maxsize=None)
def library_variants(lib=LIB):
    """Every cycle-kernel instantiation of the library, each once, sorted by name.  A code object that holds the kernels of more than one
    (I/O type, nullspace module) pair is a heavy object (the Makefile compiles every other one per joint count, I/O type and module)."""
    found = {}
    for syms in _code_objects(lib):
        names = [m.group(1) for m in (_SYM.search(s) for s in syms) if m]
        if not names:
            continue
        heavy = len({group_of(parse(n))[1:] for n in names}) > 1
        for n in names:
            v = parse(n + HEAVY if heavy else n)
            assert not v.args.get("RESERVED", False), "%s: the reserved template slot is true" % n
            if v.name in found or (n if heavy else n + HEAVY) in found:
                raise AssertionError("%s is in two code objects of the library" % n)
            found[v.name] = v
    return tuple(found[k] for k in sorted(found))


def by_group(lib=LIB):
    g = collections.defaultdict(list)
    for v in library_variants(lib):
        g[group_of(v)].append(v)
    return dict(g)


def resusage_counts(csrc=CSRC):
    """The build's per-object resource reports (nj*_kernels.resusage.txt): {object stem: {kernel template: count}} from the mangled names."""
    out = {}
    for f in glob.glob(os.path.join(csrc, "nj*_kernels.resusage.txt")):
        c = collections.Counter()
        with open(f) as fh:
            for ln in fh:
                m = re.search(r"Function Name: _ZN4vfik12_GLOBAL__N_1\d+(cycle_\w+?)I", ln)
                if m:
                    c[m.group(1)] += 1
        out[os.path.basename(f)[: -len("_kernels.resusage.txt")]] = dict(c)
    return out
