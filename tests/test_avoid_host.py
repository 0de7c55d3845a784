"""The pure host code of the whole-arm avoidance (vfclik_amd/csrc/vfik_links.h: avoid_check, avoid_rule_check) on the CPU.

(a) tests/c_host/avoid.cpp -- built here with hipcc as plain C++: no HIP header, no GPU, no library -- answers a request with the check's
    return code and reason: everything vfik_link_avoid and vfik_set_avoid_rule accept and refuse on their numbers.
(b) the same source built with -fsanitize=address,undefined and run as a program of its own (its own main; nothing is loaded into Python,
    nothing is preloaded) answers the same requests with the same bytes and no finding."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_STATE = -1, -4


def _build(tmp, name, *flags):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp / name)
    # -x c++: no HIP mode, so nothing of HIP is included behind the source's back
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags,
                           os.path.join(ROOT, "tests", "c_host", "avoid.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("avoid"), "avoid")


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("avoid_san"), "avoid_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _call(L=5, q=1, pts=4096, out=1, n_rep=8, first=2, count=5, mask=None, gain=1.0, d0=0.1, channel=-1, ext=0):
    return "call L=%d q=%d pts=%d out=%d n_rep=%d first=%d count=%d mask=%s gain=%r d0=%r channel=%d ext=%d" % (
        L, q, pts, out, n_rep, first, count, "null" if mask is None else np.asarray(mask, dtype="<u4").tobytes().hex(), float(gain), float(d0),
        channel, ext)


def _rule(L=5, gain=1.0, d0=0.1, channel=4, reserved=0, mask=None):
    m = np.zeros(16, dtype="<u4")
    if mask is not None:
        m[:len(mask)] = mask
    return "rule L=%d gain=%r d0=%r channel=%d reserved=%d mask=%s" % (L, float(gain), float(d0), channel, reserved, m.tobytes().hex())


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


def _accepted():
    full = np.full(5, 0x1F, dtype=np.uint32)
    return [("plain", _call()), ("masked", _call(mask=full)), ("negative gain", _call(gain=-2.5)), ("gain 0", _call(gain=0.0)),
            ("tiny d0", _call(d0=1e-300)), ("count 32, bit 31", _call(L=1, n_rep=32, first=0, count=32, mask=[0x80000001])),
            ("channel 3", _call(channel=3, ext=1)), ("channel 5, no out", _call(channel=5, ext=1, out=0)),
            ("16 spheres", _call(L=16, mask=np.full(16, 0x1F, dtype=np.uint32))),
            ("rule", _rule()), ("rule channel 3", _rule(channel=3)), ("rule channel 5", _rule(channel=5)),
            ("rule masked", _rule(mask=[0x1F, 0x01, 0x10, 0, 0x0A])), ("rule 16 spheres", _rule(L=16, mask=[0xFFFF] * 16)),
            ("rule negative gain", _rule(gain=-1.0))]


def _refusals():
    """(what, rc, request): everything the two entry points refuse on their numbers"""
    full = np.full(5, 0x1F, dtype=np.uint32)
    bad = [("count 0", E_ARG, _call(count=0)), ("count 33", E_ARG, _call(n_rep=40, first=0, count=33)), ("first -1", E_ARG, _call(first=-1)),
           ("first + count > n_rep", E_ARG, _call(n_rep=6)), ("first + count overflows", E_ARG, _call(first=2147483647)),
           ("q NULL", E_ARG, _call(q=0)), ("pts4 NULL", E_ARG, _call(pts=0)), ("pts4 + 8", E_ARG, _call(pts=4096 + 8)),
           ("neither out nor a channel", E_ARG, _call(out=0)), ("no spheres", E_STATE, _call(L=0)),
           ("d0 0", E_ARG, _call(d0=0.0)), ("d0 negative", E_ARG, _call(d0=-0.1)), ("d0 inf", E_ARG, _call(d0=float("inf"))),
           ("d0 nan", E_ARG, _call(d0=float("nan"))), ("gain inf", E_ARG, _call(gain=float("-inf"))), ("gain nan", E_ARG, _call(gain=float("nan"))),
           ("channel 2", E_ARG, _call(channel=2, ext=1)), ("channel 0", E_ARG, _call(channel=0, ext=1)), ("channel 6", E_ARG, _call(channel=6, ext=1)),
           ("channel -2", E_ARG, _call(channel=-2, ext=1)), ("channel 4, no ext buffer", E_STATE, _call(channel=4, ext=0)),
           ("channel 4, no ext buffer, no out", E_STATE, _call(channel=4, ext=0, out=0)),
           ("rule d0 0", E_ARG, _rule(d0=0.0)), ("rule d0 nan", E_ARG, _rule(d0=float("nan"))), ("rule d0 inf", E_ARG, _rule(d0=float("inf"))),
           ("rule gain nan", E_ARG, _rule(gain=float("nan"))), ("rule gain inf", E_ARG, _rule(gain=float("inf"))),
           ("rule channel -1", E_ARG, _rule(channel=-1)), ("rule channel 2", E_ARG, _rule(channel=2)), ("rule channel 6", E_ARG, _rule(channel=6)),
           ("rule reserved", E_ARG, _rule(reserved=1)), ("rule mask bit L", E_ARG, _rule(mask=[0x1F, 1 << 5])),
           ("rule mask word L", E_ARG, _rule(mask=[1, 1, 1, 1, 1, 1]))]
    for i in (0, 4):
        m = full.copy()
        m[i] |= 1 << 5
        bad.append(("mask[%d] bit count" % i, E_ARG, _call(mask=m)))
    return bad


def test_accepted(plain):
    ok = _accepted()
    for (what, _rq), (rc, rest) in zip(ok, _ask(plain, [rq for _w, rq in ok])):
        assert rc == 0 and rest == "msg=", (what, rc, rest)


def test_refusals(plain):
    bad = _refusals()
    for (what, want, _rq), (rc, rest) in zip(bad, _ask(plain, [rq for _w, _rc, rq in bad])):
        assert rc == want and rest.startswith("msg=") and len(rest) > 4, (what, rc, rest)


def test_sanitized_program_runs_clean(plain, sanitized):
    lines = [rq for _w, rq in _accepted()] + [rq for _w, _rc, rq in _refusals()]
    assert _ask(sanitized, lines) == _ask(plain, lines)
