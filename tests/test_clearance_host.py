"""The clearance's pure host code (vfclik_amd/csrc/vfik_links.h: clear_check, clear_mask) on the CPU.

(a) tests/c_host/clearance.cpp -- built here with hipcc as plain C++: no HIP header, no GPU, no library -- answers a request with the pair
    mask as clear_kernel reads it: permuted to the image's sorted order, sorted[i] = mask[perm[i]].  Checked against a NumPy restatement
    (a stable argsort by link), for the unsorted list with two spheres on one link among others, with and without a mask; and every
    refusal vfik_link_clearance documents.
(b) the same source built with -fsanitize=address,undefined and run as a program of its own (its own main; nothing is loaded into Python,
    nothing is preloaded) answers the same requests with the same bytes and no finding."""
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
ML = _abi.MAX_LINK_SPHERES
SPHERE = np.dtype([("link", "<i4"), ("reserved", "<i4"), ("c", "<f8", (3,)), ("radius", "<f8")])   # vfik_link_sphere
E_ARG, E_STATE = -1, -4


def _build(tmp, name, *flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp / name)
    # -x c++: no HIP mode, so nothing of HIP is included behind the source's back
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags,
                           os.path.join(ROOT, "tests", "c_host", "clearance.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("clearance"), "clearance")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("clearance_san"), "clearance_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _spheres(items):
    s = np.zeros(len(items), dtype=SPHERE)
    for k, it in enumerate(items):
        s[k]["link"], s[k]["c"], s[k]["radius"] = it[0], it[1], it[2]
    return s


def _request(chain, items, n_rep, first, count, mask=None, q=1, pts=4096, clear=1):
    s = _spheres(items)
    return "chain=%s spheres=%s q=%d pts=%d clear=%d n_rep=%d first=%d count=%d mask=%s" % (
        bytes(chain.to_struct()).hex(), s.tobytes().hex() if len(items) else "none", q, pts, clear, n_rep, first, count,
        "null" if mask is None else np.asarray(mask, dtype="<u4").tobytes().hex())


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


def _sorted_mask(rest):
    assert rest.startswith("mask=")
    raw = bytes.fromhex(rest[5:])
    assert len(raw) == 4 * ML
    return np.frombuffer(raw, dtype="<u4")


def _restated(items, mask, count):
    """NumPy: the caller's words in the order of a stable sort by link; every row where there is no mask; zeros from L on"""
    L = len(items)
    perm = np.argsort([it[0] for it in items], kind="stable")
    all_rows = np.uint32(0xFFFFFFFF if count == 32 else (1 << count) - 1)
    out = np.zeros(ML, dtype=np.uint32)
    out[:L] = all_rows if mask is None else np.asarray(mask, dtype=np.uint32)[perm]
    return out


def _accepted():
    """(name, chain, items, n_rep, first, count, mask)"""
    out = []
    rng = np.random.default_rng(41)
    for robot in hl.ROBOTS:
        ch = hl.chain_of(robot)
        for kind in hl.SPHERE_LISTS:
            items = hl.sphere_list(ch, kind)
            for count, first in ((1, 0), (5, 3), (16, 0), (32, 3)):
                mask = rng.integers(0, 1 << count, size=len(items), dtype=np.uint64).astype(np.uint32)
                out.append(("%s-%s-%d" % (robot, kind, count), ch, items, first + count + 2, first, count, mask))
                out.append(("%s-%s-%d-all" % (robot, kind, count), ch, items, first + count, first, count, None))
    lwr = robots.lwr()
    ties = [(5, (0.1, 0, 0), 0.01), (7, (0, 0.2, 0), 0.02), (5, (0.3, 0, 0), 0.03), (0, (0, 0, 0.4), 0.0), (5, (0.5, 0, 0), 0.05), (7, (0, 0.6, 0), 0.06)]
    out.append(("lwr-ties", lwr, ties, 8, 0, 8, np.array([0x01, 0x02, 0x04, 0x08, 0x10, 0x20], dtype=np.uint32)))
    return out


def _refusals():
    """(what, rc, request): everything vfik_link_clearance refuses"""
    lwr = robots.lwr()
    items = hl.sphere_list(lwr, "five")
    ok = dict(n_rep=8, first=2, count=5)
    full = np.full(5, 0x1F, dtype=np.uint32)
    bad = [("count 0", E_ARG, _request(lwr, items, 8, 2, 0)),
           ("count -1", E_ARG, _request(lwr, items, 8, 2, -1)),
           ("count 33", E_ARG, _request(lwr, items, 40, 0, 33)),
           ("first -1", E_ARG, _request(lwr, items, 8, -1, 5)),
           ("first + count > n_rep", E_ARG, _request(lwr, items, 6, 2, 5)),
           ("first + count overflows", E_ARG, _request(lwr, items, 8, 2147483647, 5)),
           ("q NULL", E_ARG, _request(lwr, items, q=0, **ok)),
           ("pts4 NULL", E_ARG, _request(lwr, items, pts=0, **ok)),
           ("clear NULL", E_ARG, _request(lwr, items, clear=0, **ok)),
           ("pts4 + 8", E_ARG, _request(lwr, items, pts=4096 + 8, **ok)),
           ("pts4 + 4", E_ARG, _request(lwr, items, pts=4096 + 4, **ok)),
           ("no spheres", E_STATE, _request(lwr, [], **ok))]
    for i in (0, 4):
        m = full.copy()
        m[i] |= 1 << 5
        bad.append(("mask[%d] bit count" % i, E_ARG, _request(lwr, items, mask=m, **ok)))
        m = full.copy()
        m[i] |= 1 << 31
        bad.append(("mask[%d] bit 31" % i, E_ARG, _request(lwr, items, mask=m, **ok)))
    return bad


def test_mask_in_the_images_order(plain):
    cases = _accepted()
    ans = _ask(plain, [_request(ch, items, n_rep, first, count, mask) for _n, ch, items, n_rep, first, count, mask in cases])
    for (name, _ch, items, _n_rep, _first, count, mask), (rc, rest) in zip(cases, ans):
        assert rc == 0, (name, rest)
        assert np.array_equal(_sorted_mask(rest), _restated(items, mask, count)), name
    # the list with ties, spelled out: links 0 5 5 5 7 7 from the caller's 3 0 2 4 1 5
    assert list(_sorted_mask(ans[-1][1])[:7]) == [0x08, 0x01, 0x04, 0x10, 0x02, 0x20, 0]
    # a mask that names every row of a full window is accepted: bit 31 at count 32
    lwr = robots.lwr()
    rc, rest = _ask(plain, [_request(lwr, hl.sphere_list(lwr, "one"), 32, 0, 32, np.array([0x80000001], dtype=np.uint32))])[0]
    assert rc == 0 and _sorted_mask(rest)[0] == 0x80000001


def test_refusals(plain):
    bad = _refusals()
    for (what, want, _rq), (rc, rest) in zip(bad, _ask(plain, [rq for _w, _rc, rq in bad])):
        assert rc == want and rest.startswith("msg=") and len(rest) > 4, (what, rc, rest)


def test_sanitized_program_runs_clean(plain, sanitized):
    lines = [_request(ch, items, n_rep, first, count, mask) for _n, ch, items, n_rep, first, count, mask in _accepted()]
    lines += [rq for _w, _rc, rq in _refusals()]
    assert _ask(sanitized, lines) == _ask(plain, lines)
