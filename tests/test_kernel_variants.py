"""The cycle-kernel variants the built library ships (tests/kernel_variants.py reads them from libvfik_hip.so), checked on the CPU:
every name parses, the joint counts are the library's own, the build's resource reports agree object by object, and every kernel a
route of the launch plan names (tests/test_launch_plan.py: ROUTES) is linked in -- a plan that names an instantiation that was not
built would otherwise only show at run time, as hipErrorInvalidDeviceFunction."""
import collections
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_variants as kv  # noqa: E402
from test_launch_plan import ROUTES  # noqa: E402


@pytest.fixture(scope="module")
def variants():
    import __graft_entry__ as g
    g.build()
    return kv.library_variants()


def test_every_cycle_kernel_of_the_library_parses(variants):
    assert len(variants) > 100
    for v in variants:
        assert kv.parse(v.name) == v
        assert v.args["T"] in ("float", "double") and isinstance(v.args["NS"], bool)
        assert v.heavy == (v.kernel == "cycle_kernel_x" and v.args["NJ"] >= 12 and v.args["LEAN"] == 0 and not v.args["ROLL"]), v.name


def test_joint_counts_are_those_the_library_supports(variants):
    from vfclik_amd import engine
    mask = engine.load_library().vfik_supported_joints()
    supported = {n for n in range(32) if (mask >> n) & 1}
    groups = {kv.group_of(v) for v in variants}
    assert {g[0] for g in groups} == supported
    # one object per (joint count, I/O type, nullspace module): every one of them holds cycle kernels
    assert groups == {(n, t, ns) for n in supported for t in (32, 64) for ns in (False, True)}


def test_the_build_reports_agree_with_the_library(variants):
    """The per-object resource reports the build writes (csrc/Makefile, RESUSAGE) count the same kernels per object."""
    reports = kv.resusage_counts()
    assert reports, "no nj*_kernels.resusage.txt beside the library"
    lib = collections.defaultdict(collections.Counter)
    for v in variants:
        n, t, ns = kv.group_of(v)
        lib["nj%d_heavy" % n if v.heavy else "nj%d_t%d_ns%d" % (n, t, int(ns))][v.kernel] += 1
    assert {k: dict(c) for k, c in lib.items()} == reports


def test_every_kernel_a_route_names_is_built(variants):
    names = {v.name for v in variants}
    routed = {o.split(" grid=")[0] for _, o in ROUTES} - {"refused"}
    assert len(routed) > 40
    missing = sorted(routed - names)
    assert not missing, "planned but not built:\n" + "\n".join(missing)


def test_parse_refuses_what_is_not_a_cycle_kernel():
    for bad in ("mix_kernel<float>", "cycle_kernel_m<float, 7, true, 1, false>", "cycle_kernel_s<half, 7, true, true, false, true, 1, -1, false, false, 1, false, 0>"):
        with pytest.raises(ValueError):
            kv.parse(bad)
