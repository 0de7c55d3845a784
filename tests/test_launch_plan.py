"""The launch plan of the cycle kernel (vfclik_amd/csrc/vfik_kernel.h: plan_cycle), pinned route by route: a host driver
(tests/c_host/launch_plan.cpp, built with hipcc as host code -- no GPU, no library) prints the kernel instantiation each launch
description takes, with its grid, block and LDS bytes.  Every route of the dispatch is in the table: each kernel family, the FUN /
UNI / MIXO variants and the nullspace module's flag sets as compile-time constants, the DH-pattern bits and the cases that drop
them, both I/O types, 6 / 7 / 10 / 14 joints, the eight-lanes kernel's caps on both sides, launches of more and fewer waves than
the device has SIMDs, the two-waves build, the long chains' heavy object and the in-kernel / stepped rollout.

A row: the launch (KArgs members; pointers 1 = given; defaults in the driver: 7 joints, float32 I/O, 4 096 arms, 256 threads a
block, the straight-line field path, PLAIN, 1 024 SIMDs, the shipped eight-lanes caps), then what it takes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROUTES = [
    ('nj=7 io=32 B=64 pose=1',
     'cycle_sub8_kernel_x<float, 7, false, 0> grid=8 block=64 lds=8192'),
    ('nj=7 io=32 B=64 pose=1 dhp=1',
     'cycle_sub8_kernel_x<float, 7, false, 1> grid=8 block=64 lds=8192'),
    ('nj=7 io=32 B=4096 pose=1 dhp=1 plain=2',
     'cycle_sub8_kernel_x<float, 7, false, 3> grid=512 block=64 lds=8192'),
    ('nj=7 io=32 B=64 qdist=1 dhp=1 plain=3',
     'cycle_sub8_kernel_x<float, 7, false, 5> grid=8 block=64 lds=8192'),
    ('nj=7 io=32 B=64 pose=1 dhp=1 plain=4',
     'cycle_sub8_kernel_x<float, 7, false, 7> grid=8 block=64 lds=8192'),
    ('nj=6 io=64 B=64 pose=1 dhp=1',
     'cycle_sub8_kernel_x<double, 6, false, 1> grid=8 block=64 lds=8192'),
    ('nj=7 io=64 B=64 pose=1 dhp=1 plain=4',
     'cycle_sub8_kernel_x<double, 7, false, 7> grid=8 block=64 lds=8192'),
    ('nj=7 io=32 B=16 flags=5 sub8_ns=32 dhp=1',
     'cycle_sub8_kernel<float, 7, true, 1> grid=2 block=64 lds=8192'),
    ('nj=7 io=32 B=33 flags=5 sub8_ns=32 dhp=1',
     'cycle_kernel_s<float, 7, true, true, false, true, 1, 5, false, false, 1, false, 1> grid=1 block=256 lds=80896'),
    ('nj=7 io=32 B=4097 pose=1 dhp=1',
     'cycle_kernel_x<float, 7, false, true, false, true, 3, -1, false, false, 1, false, false, 1> grid=17 block=256 lds=80896'),
    ('nj=7 io=32 B=64 sub8=0',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, false, 0> grid=1 block=256 lds=80896'),
    ('nj=7 io=32 B=64 sub8=64 dhp=1',
     'cycle_sub8_kernel_x<float, 7, false, 1> grid=8 block=64 lds=8192'),
    ('nj=7 io=32 B=65 sub8=64 dhp=1',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, false, 1> grid=1 block=256 lds=80896'),
    ('nj=7 io=32 B=65536',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, false, 0> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 dhp=1',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, false, 1> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 dhp=1 uni=1',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, true, 1> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 dhp=1 flags=5',
     'cycle_kernel_s<float, 7, true, true, false, true, 1, 5, false, false, 1, false, 1> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 dhp=1 flags=5 uni=1',
     'cycle_kernel_s<float, 7, true, true, false, true, 1, 5, false, false, 1, true, 1> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 dhp=1 flags=7 uni=1',
     'cycle_kernel_s<float, 7, true, true, false, true, 1, 7, false, false, 1, true, 1> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 flags=1',
     'cycle_kernel_s<float, 7, true, true, false, true, 1, -1, false, false, 1, false, 0> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 dhp=1 funnel=1',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, true, 1, false, 1> grid=256 block=256 lds=105472'),
    ('nj=7 io=32 B=65536 dhp=1 plain=2',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, false, 3> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 dhp=1 plain=2 funnel=1',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, true, 1, false, 3> grid=256 block=256 lds=105472'),
    ('nj=7 io=32 B=65536 dhp=1 plain=3 uni=1',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, true, 5> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 dhp=1 plain=4',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, false, 7> grid=256 block=256 lds=80896'),
    # the rule for a shared tool's 3 x 3 block (include/vfik.h, vfik_set_tool; the driver takes plain and dhp from kconst_fill on the LWR with that tool): a block off a rotation
    # by 1e-4 (typed with four decimals), and one at 0.062 -- below VFIK_TOOL_MAX_DEFECT = 1/16 -- stay plain + tool handles ...
    ('nj=7 io=32 B=65536 dhp=1 plain=2 tool_shear_e6=100',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, false, 3> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 dhp=1 plain=2 tool_shear_e6=62000',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, false, 3> grid=256 block=256 lds=80896'),
    # ... one beyond it, and a block without an inverse (last column zero), take the general variants, which need no inverse
    ('nj=7 io=32 B=65536 dhp=1 plain=2 tool_shear_e6=63000',
     'cycle_kernel_x<float, 7, false, false, false, true, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=117760'),
    ('nj=7 io=32 B=65536 dhp=1 plain=2 tool_flat=1',
     'cycle_kernel_x<float, 7, false, false, false, true, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=117760'),
    ('nj=7 io=64 B=64 pose=1 pose_nt=1 dhp=1 plain=2 tool_shear_e6=100',
     'cycle_sub8_kernel_x<double, 7, false, 3> grid=8 block=64 lds=8192'),
    ('nj=7 io=64 B=64 pose=1 pose_nt=1 dhp=1 plain=2 tool_flat=1',
     'cycle_kernel_x<double, 7, false, false, false, true, 0, -1, false, false, 1, false, false, 0> grid=1 block=256 lds=161792'),
    ('nj=7 io=32 B=65536 dhp=0 plain=2',
     'cycle_kernel_x<float, 7, false, false, false, true, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=117760'),
    ('nj=7 io=32 B=131072 dhp=1',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, false, 1> grid=512 block=256 lds=117760'),
    ('nj=7 io=32 B=131072 dhp=1 plain=2',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 1, false, 3> grid=512 block=256 lds=117760'),
    ('nj=7 io=32 B=131072 dhp=1 waves2=1',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 2, false, 0> grid=512 block=256 lds=80896'),
    ('nj=7 io=32 B=131072 dhp=1 waves2=1 uni=1',
     'cycle_kernel_s<float, 7, false, true, false, true, 1, -1, false, false, 2, true, 1> grid=512 block=256 lds=80896'),
    ('nj=7 io=32 B=131072 dhp=1 waves2=1 uni=1 flags=5',
     'cycle_kernel_s<float, 7, true, true, false, true, 1, 5, false, false, 2, true, 1> grid=512 block=256 lds=80896'),
    ('nj=7 io=32 B=131072 dhp=1 waves2=1 uni=1 flags=7',
     'cycle_kernel_s<float, 7, true, true, false, true, 1, 7, false, false, 2, true, 1> grid=512 block=256 lds=80896'),
    ('nj=7 io=32 B=131072 dhp=1 waves2=1 uni=1 flags=1',
     'cycle_kernel_s<float, 7, true, true, false, true, 1, -1, false, false, 2, true, 1> grid=512 block=256 lds=80896'),
    ('nj=7 io=32 B=131072 dhp=1 waves2=1 flags=5',
     'cycle_kernel_s<float, 7, true, true, false, true, 1, 5, false, false, 1, false, 1> grid=512 block=256 lds=117760'),
    ('nj=6 io=32 B=65536 dhp=1',
     'cycle_kernel_s<float, 6, false, true, false, true, 1, -1, false, false, 1, false, 1> grid=256 block=256 lds=79872'),
    ('nj=6 io=64 B=65536 dhp=1',
     'cycle_kernel_s<double, 6, false, true, false, true, 1, -1, false, false, 1, false, 0> grid=256 block=256 lds=102400'),
    ('nj=7 io=64 B=65536 dhp=1',
     'cycle_kernel_s<double, 7, false, true, false, true, 1, -1, false, false, 1, false, 1> grid=256 block=256 lds=104448'),
    ('nj=7 io=64 B=65536 dhp=1 flags=7 uni=1',
     'cycle_kernel_s<double, 7, true, true, false, true, 1, 7, false, false, 1, true, 1> grid=256 block=256 lds=104448'),
    ('nj=7 io=64 B=65536 dhp=1 plain=2',
     'cycle_kernel_x<double, 7, false, false, false, true, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=161792'),
    ('nj=10 io=32 B=65536',
     'cycle_kernel_s<float, 10, false, true, false, true, 1, -1, false, false, 1, false, 0> grid=256 block=256 lds=88064'),
    ('nj=10 io=32 B=65536 plain=2',
     'cycle_kernel_s<float, 10, false, true, false, true, 1, -1, false, false, 1, false, 2> grid=256 block=256 lds=88064'),
    ('nj=10 io=32 B=65536 plain=3',
     'cycle_kernel_x<float, 10, false, false, false, true, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=124928'),
    ('nj=14 io=32 B=65536 dhp=1',
     'cycle_kernel_s<float, 14, false, true, false, true, 1, -1, false, false, 1, false, 1> grid=256 block=256 lds=92160'),
    ('nj=14 io=32 B=65536 dhp=1 plain=2',
     'cycle_kernel_s<float, 14, false, true, false, true, 1, -1, false, false, 1, false, 3> grid=256 block=256 lds=92160'),
    ('nj=14 io=64 B=65536 dhp=1',
     'cycle_kernel_s<double, 14, false, true, false, true, 1, -1, false, false, 1, false, 0> grid=1024 block=64 lds=30720'),
    ('nj=7 io=32 B=65536 pose=1 dhp=1',
     'cycle_kernel_x<float, 7, false, true, false, true, 3, -1, false, false, 1, false, false, 1> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 pose=1 qdot_vf=1 qdot_null=1 null_control=1 flags=5 dhp=1 uni=1',
     'cycle_kernel_x<float, 7, true, true, false, true, 3, 5, false, false, 1, true, false, 1> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 pose=1 flags=7 dhp=1',
     'cycle_kernel_x<float, 7, true, true, false, true, 3, 7, false, false, 1, false, false, 1> grid=256 block=256 lds=80896'),
    ('nj=7 io=32 B=65536 v6=1 goal_dist=1 active=1 dhp=1 funnel=1',
     'cycle_kernel_x<float, 7, false, true, false, true, 3, -1, false, true, 1, false, false, 1> grid=256 block=256 lds=105472'),
    ('nj=7 io=32 B=65536 pose=1 dhp=1 plain=2 uni=1',
     'cycle_kernel_x<float, 7, false, true, false, true, 3, -1, false, false, 1, true, false, 3> grid=256 block=256 lds=80896'),
    ('nj=7 io=64 B=65536 pose=1 dhp=1',
     'cycle_kernel_x<double, 7, false, true, false, true, 3, -1, false, false, 1, false, false, 1> grid=256 block=256 lds=104448'),
    ('nj=14 io=64 B=65536 pose=1 dhp=1',
     'cycle_kernel_x<double, 14, false, true, false, true, 3, -1, false, false, 1, false, false, 0> grid=1024 block=64 lds=30720'),
    ('nj=14 io=32 B=65536 pose=1 dhp=1 plain=2',
     'cycle_kernel_x<float, 14, false, true, false, true, 3, -1, false, false, 1, false, false, 3> grid=256 block=256 lds=92160'),
    ('nj=7 io=32 B=65536 mixed=1 dhp=1',
     'cycle_kernel_m<float, 7, false, 1, false, 1> grid=1024 block=64 lds=21248'),
    ('nj=7 io=32 B=4096 mixed=1 dhp=1',
     'cycle_kernel_m<float, 7, false, 1, false, 1> grid=64 block=64 lds=21248'),
    ('nj=7 io=32 B=65536 mixed=1 pose=1 dhp=1',
     'cycle_kernel_m<float, 7, false, 3, false, 1> grid=1024 block=64 lds=21248'),
    ('nj=7 io=32 B=4096 mixed=1 funnel=1 dhp=1',
     'cycle_kernel_m<float, 7, false, 1, true, 1> grid=64 block=64 lds=27392'),
    ('nj=7 io=32 B=65536 mixed=1 dhp=1 plain=3',
     'cycle_kernel_m<float, 7, false, 1, false, 5> grid=1024 block=64 lds=21248'),
    ('nj=7 io=64 B=65536 mixed=1 dhp=1',
     'cycle_kernel_m<double, 7, false, 1, false, 1> grid=1024 block=64 lds=27136'),
    ('nj=14 io=64 B=4096 mixed=1 dhp=1 pose=1',
     'cycle_kernel_m<double, 14, false, 3, false, 0> grid=64 block=64 lds=31744'),
    ('nj=7 io=32 B=65536 mixed=1 q_ref=1',
     'cycle_kernel_x<float, 7, false, true, false, false, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=117760'),
    ('nj=7 io=32 B=4096 n_cycles=50 q_out=1 dhp=1',
     'cycle_kernel_x<float, 7, false, true, true, true, 1, -1, false, false, 1, false, false, 1> grid=16 block=256 lds=80896'),
    ('nj=7 io=64 B=4096 n_cycles=50 q_out=1 dhp=1',
     'cycle_kernel_x<double, 7, false, true, true, true, 1, -1, false, false, 1, false, false, 1> grid=16 block=256 lds=104448'),
    ('nj=7 io=32 B=4096 n_cycles=50 pose=1 dhp=1',
     'cycle_kernel_x<float, 7, false, true, true, true, 0, -1, false, false, 1, false, false, 0> grid=16 block=256 lds=117760'),
    ('nj=7 io=32 B=4096 n_cycles=50 fast_order=-1',
     'cycle_kernel_x<float, 7, false, true, true, false, 0, -1, false, false, 1, false, false, 0> grid=16 block=256 lds=117760'),
    ('nj=7 io=32 B=4096 n_cycles=50 funnel=1',
     'cycle_kernel_x<float, 7, false, true, true, false, 0, -1, false, false, 1, false, false, 0> grid=16 block=256 lds=117760'),
    ('nj=7 io=32 B=4096 n_cycles=50 plain=2 dhp=1',
     'refused grid=16 block=256 lds=117760'),
    ('nj=7 io=32 B=4096 n_cycles=50 plain=0',
     'refused grid=16 block=256 lds=117760'),
    ('nj=10 io=32 B=4096 n_cycles=50',
     'refused grid=16 block=256 lds=124928'),
    ('nj=14 io=32 B=4096 q_out=1 dhp=1',
     'cycle_kernel_x<float, 14, false, true, false, true, 2, -1, false, false, 1, false, false, 1> grid=16 block=256 lds=92160'),
    ('nj=14 io=64 B=4096 q_out=1 dhp=1',
     'cycle_kernel_x<double, 14, false, true, false, true, 2, -1, false, false, 1, false, false, 0> grid=64 block=64 lds=30720'),
    ('nj=10 io=32 B=4096 q_out=1',
     'cycle_kernel_x<float, 10, false, true, false, true, 2, -1, false, false, 1, false, false, 0> grid=16 block=256 lds=88064'),
    ('nj=7 io=32 B=4096 q_out=1 dhp=1 plain=2',
     'cycle_kernel_x<float, 7, false, false, false, true, 0, -1, false, false, 1, false, false, 0> grid=16 block=256 lds=117760'),
    ('nj=7 io=32 B=65536 fast_order=-1 dhp=1',
     'cycle_kernel_x<float, 7, false, true, false, false, 1, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=117760'),
    ('nj=14 io=64 B=65536 fast_order=-1',
     'cycle_kernel_x<double, 14, false, true, false, false, 1, -1, false, false, 1, false, false, 0> grid=1024 block=64 lds=34816'),
    ('nj=7 io=32 B=65536 funnel=1 q_ref=1 dhp=1',
     'cycle_kernel_x<float, 7, false, true, false, false, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=117760'),
    ('nj=7 io=32 B=65536 plain=0 tool=1',
     'cycle_kernel_x<float, 7, false, false, false, true, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=117760'),
    ('nj=7 io=32 B=65536 plain=0 fast_order=-1 mixw=1',
     'cycle_kernel_x<float, 7, false, false, false, false, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=117760'),
    ('nj=7 io=32 B=65536 q_ref=1 q_ref_out=1 dhp=1',
     'cycle_kernel_x<float, 7, false, true, false, true, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=117760'),
    ('nj=7 io=32 B=65536 q_lo=1 plain=2 dhp=1',
     'cycle_kernel_x<float, 7, false, false, false, true, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=117760'),
    ('nj=7 io=64 B=65536 plain=4 dhp=1',
     'cycle_kernel_x<double, 7, false, false, false, true, 0, -1, false, false, 1, false, false, 0> grid=256 block=256 lds=161792'),
    ('nj=14 io=64 B=65536 plain=0 tool=1',
     'cycle_kernel_x<double, 14, false, false, false, true, 0, -1, false, false, 1, false, false, 0> [heavy] grid=1024 block=64 lds=45056'),
    ('nj=14 io=64 B=65536 q_cmded=1 dhp=1',
     'cycle_kernel_x<double, 14, false, true, false, true, 0, -1, false, false, 1, false, false, 0> [heavy] grid=1024 block=64 lds=34816'),
    ('nj=14 io=32 B=65536 plain=0 fast_order=-1 wts=1 block=512',
     'cycle_kernel_x<float, 14, false, false, false, false, 0, -1, false, false, 1, false, false, 0> [heavy] grid=205 block=320 lds=161280'),
    ('nj=10 io=64 B=65536 ext=1',
     'cycle_kernel_x<double, 10, false, true, false, true, 0, -1, false, false, 1, false, false, 0> grid=1024 block=64 lds=32768'),
    ('nj=7 io=32 B=65536 block=1024 pose=1',
     'cycle_kernel_x<float, 7, false, true, false, true, 3, -1, false, false, 1, false, false, 0> grid=205 block=320 lds=147200'),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c_host", "launch_plan.cpp"), "-o", exe])
    return exe


def test_every_route_takes_the_kernel_it_took(driver):
    r = subprocess.run([driver], input="\n".join(c for c, _ in ROUTES) + "\n", capture_output=True, text=True, timeout=60, check=True)
    got = r.stdout.splitlines()
    assert len(got) == len(ROUTES)
    diff = ["%s\n    want %s\n    got  %s" % (c, w, g) for (c, w), g in zip(ROUTES, got) if w != g]
    assert not diff, "\n".join(diff)


def test_the_table_reaches_every_family():
    kernels = {o.split("<")[0].split()[0] for _, o in ROUTES}
    assert kernels == {"cycle_sub8_kernel", "cycle_sub8_kernel_x", "cycle_kernel_s", "cycle_kernel_x", "cycle_kernel_m", "refused"}
    assert any("[heavy]" in o for _, o in ROUTES)
    for lean, roll in ((", true, true, true, 1,", "rollout, lean"), (", true, true, true, 0,", "rollout"), (", true, true, false, 0,", "rollout, general path"),
                       (", true, false, true, 2,", "stepped cycle"), (", true, false, false, 1,", "general-path lean"), (", true, false, true, 3,", "publishing lean")):
        assert any(o.startswith("cycle_kernel_x") and lean in o for _, o in ROUTES), roll
