"""The link spheres as pure host code (vfclik_amd/csrc/vfik_links.h: links_check, links_fill) on the CPU, and the host's float64 link points
against the 50-digit ones.

(a) tests/c_host/links.cpp -- built here with hipcc as plain C++: no HIP header, no GPU, no library -- turns a vfik_chain and a list of
    vfik_link_sphere into the image link_kernel reads.  Checked: B[0..n] and jtype as they came; the spheres SORTED by link, spheres of one
    link in the caller's order; perm[] leading back to the caller's list, from an unsorted list with several spheres on one link; the tails
    of the arrays; and every refusal vfik_set_link_spheres documents.
(b) the same source built with -fsanitize=address,undefined and run as a program of its own (its own main; nothing is loaded into Python,
    nothing is preloaded) answers the same requests with the same bytes and no finding.
(c) Chain.fk of the chain truncated at a sphere's link (hp_links.host_points) against hp_links.link_points on the cases of
    tests/test_gpu_link_points.py: R, the host's worst error in units of n u reach, printed per case and held under K_MARGIN -- the GPU
    test gives the device K_MARGIN max(1, R) of the same units."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_links as hl  # noqa: E402

from vfclik_amd import _abi, robots  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MJ, ML = _abi.MAX_JOINTS, _abi.MAX_LINK_SPHERES
SPHERE = np.dtype([("link", "<i4"), ("reserved", "<i4"), ("c", "<f8", (3,)), ("radius", "<f8")])   # vfik_link_sphere
IMAGE = np.dtype([("n", "<i4"), ("L", "<i4"), ("jtype", "<i4", (MJ,)), ("link", "<i4", (ML,)), ("perm", "<i4", (ML,)),
                  ("B", "<f8", (MJ + 1, 12)), ("c", "<f8", (ML, 4))])                             # vfik::LinkImage


def _build(tmp, name, *flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp / name)
    # -x c++: no HIP mode, so nothing of HIP is included behind the source's back
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags,
                           os.path.join(ROOT, "tests", "c_host", "links.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("links"), "links")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("links_san"), "links_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _spheres(items):
    s = np.zeros(len(items), dtype=SPHERE)
    for k, it in enumerate(items):
        s[k]["link"], s[k]["c"], s[k]["radius"] = it[0], it[1], it[2]
        s[k]["reserved"] = it[3] if len(it) > 3 else 0
    return s


def _request(chain, s, L=None, null=False):
    return "chain=%s L=%d spheres=%s" % (bytes(chain.to_struct()).hex(), len(s) if L is None else L, "null" if null else s.tobytes().hex())


def _ask(exe, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out = []
    for ln in r.stdout.splitlines():
        rc, rest = ln.split(" ", 1)
        out.append((int(rc[3:]), rest))
    assert len(out) == len(lines)
    return out


def _image(rest):
    assert rest.startswith("image=")
    raw = bytes.fromhex(rest[6:])
    assert len(raw) == IMAGE.itemsize
    return np.frombuffer(raw, dtype=IMAGE)[0]


def _cases():
    """(name, chain, items) of the accepted lists: the GPU test's, an empty one, and one with three spheres on one link between others"""
    out = []
    for robot in hl.ROBOTS:
        ch = hl.chain_of(robot)
        for kind in hl.SPHERE_LISTS:
            out.append(("%s-%s" % (robot, kind), ch, hl.sphere_list(ch, kind)))
    lwr = robots.lwr()
    out.append(("lwr-none", lwr, []))
    out.append(("lwr-ties", lwr, [(5, (0.1, 0, 0), 0.01), (7, (0, 0.2, 0), 0.02), (5, (0.3, 0, 0), 0.03), (0, (0, 0, 0.4), 0.0), (5, (0.5, 0, 0), 0.05),
                                  (7, (0, 0.6, 0), 0.06)]))
    return out


def _check_image(img, chain, items):
    n, L = chain.n, len(items)
    assert img["n"] == n and img["L"] == L
    assert list(img["jtype"][:n]) == chain.jtype and not img["jtype"][n:].any()
    assert np.array_equal(img["B"][: n + 1], chain.B.reshape(n + 1, 12)) and not img["B"][n + 1:].any()
    link, perm = img["link"], img["perm"]
    assert np.all(np.diff(link[:L]) >= 0), link                       # sorted by link
    assert sorted(perm[:L]) == list(range(L))                         # a permutation of the caller's list
    for i in range(L):
        lk, c, r = items[perm[i]][:3]
        assert link[i] == lk and np.array_equal(img["c"][i], [c[0], c[1], c[2], r])
        if i and link[i] == link[i - 1]:
            assert perm[i] > perm[i - 1]                              # spheres of one link keep the caller's order
    assert np.all(link[L:] == -1) and not perm[L:].any() and not img["c"][L:].any()


def _refusals():
    """(what, request): every list vfik_set_link_spheres refuses with VFIK_E_ARG"""
    lwr = robots.lwr()
    ok = (3, (0.1, 0.2, 0.3), 0.05)
    bad = [("L 17", _request(lwr, _spheres([ok] * 17))),
           ("L -1", _request(lwr, _spheres([ok]), L=-1)),
           ("L 2 and no list", _request(lwr, _spheres([]), L=2, null=True)),
           ("link -1", _request(lwr, _spheres([ok, (-1, ok[1], ok[2])]))),
           ("link n + 1", _request(lwr, _spheres([(8, ok[1], ok[2]), ok]))),
           ("reserved", _request(lwr, _spheres([ok, (3, ok[1], ok[2], 1)])))]
    for k in range(3):
        for v in (np.nan, np.inf, -np.inf):
            c = list(ok[1])
            c[k] = v
            bad.append(("centre[%d] %s" % (k, v), _request(lwr, _spheres([ok, (3, tuple(c), 0.05)]))))
    for v in (-1e-300, -0.05, np.nan, np.inf, -np.inf):
        bad.append(("radius %s" % v, _request(lwr, _spheres([(3, ok[1], v)]))))
    return bad


def test_sorted_image_and_permutation(plain):
    cases = _cases()
    ans = _ask(plain, [_request(ch, _spheres(items)) for _n, ch, items in cases])
    for (name, ch, items), (rc, rest) in zip(cases, ans):
        assert rc == 0, (name, rest)
        _check_image(_image(rest), ch, items)
    # the list with ties, spelled out: links 0 5 5 5 7 7 from the caller's 3 0 2 4 1 5
    img = _image(ans[-1][1])
    assert list(img["link"][:6]) == [0, 5, 5, 5, 7, 7] and list(img["perm"][:6]) == [3, 0, 2, 4, 1, 5]
    # a NULL list with L = 0 is "no spheres"
    rc, rest = _ask(plain, [_request(robots.lwr(), _spheres([]), L=0, null=True)])[0]
    assert rc == 0 and _image(rest)["L"] == 0
    # radius 0 and the flange are accepted
    rc, rest = _ask(plain, [_request(robots.lwr(), _spheres([(7, (0, 0, 0), 0.0)]))])[0]
    assert rc == 0 and _image(rest)["link"][0] == 7


def test_refusals(plain):
    bad = _refusals()
    for (what, _rq), (rc, rest) in zip(bad, _ask(plain, [rq for _w, rq in bad])):
        assert rc == -1 and rest.startswith("msg=") and len(rest) > 4, (what, rc, rest)


def test_sanitized_program_runs_clean(plain, sanitized):
    lines = [_request(ch, _spheres(items)) for _n, ch, items in _cases()] + [rq for _w, rq in _refusals()]
    assert _ask(sanitized, lines) == _ask(plain, lines)


@pytest.mark.parametrize("robot", hl.ROBOTS)
@pytest.mark.parametrize("io_dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_host_points_against_50_digits(robot, io_dtype):
    """R per case; B = 203 as on the GPU.  The host's float64 walk is a few roundings per link: it stays under K_MARGIN units."""
    worst = 0.0
    for kind, src, with_xform in hl.CASES:
        R, _ref = hl.host_ratio(robot, kind, src, with_xform, 203, io_dtype)
        print("%-10s %-5s %-4s xform %d  R = %.3f units of n u reach" % (robot, kind, src, with_xform, R))
        worst = max(worst, R)
    assert hl.hp.BACKEND in ("mpmath", "longdouble")
    assert worst < hl.K_MARGIN, worst
