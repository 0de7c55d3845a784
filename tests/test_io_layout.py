"""The staging layout of the host-pointer call forms (vfclik_amd/csrc/vfik_io_layout.h): tests/c_host/io_layout.cpp -- host code
only, no HIP, no library -- under AddressSanitizer + UBSan, as a process of its own.  For 6 / 7 / 16 joints, both element sizes,
1 / 37 / 700 arms and three member subsets (q and qdot_out; everything; everything plus a goto's four extras) it checks that every
present member is 256-byte aligned, that no two overlap, that the inputs are a prefix, that absent members take no room and that
the total is the sum of the rounded sizes.  The same program checks the timed moves (goto, follow, goto_js, follow_js): the table of the
arrays their host forms stage and the pure function that picks a block's rows."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def io_layout_output(tmp_path_factory):
    """The program built (with the sanitizers where their runtime exists) and run once: what it printed."""
    tmp_path = tmp_path_factory.mktemp("io_layout")
    exe = str(tmp_path / "io_layout")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "c_host", "io_layout.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", str(probe), "-o", str(tmp_path / "probe")] + san, capture_output=True).returncode != 0:
        print("no sanitizer runtime on this machine: io_layout is built WITHOUT -fsanitize")
        san = []
    r = subprocess.run(base + san, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_io_layout_under_asan_ubsan(io_layout_output):
    assert "io_layout OK (54 cases)" in io_layout_output


def test_timed_move_table_and_block_rows(io_layout_output):
    """Each of the four forms, both element sizes, n in {6, 7, 16}, B in {1, 37, 700}, W in {1, 3}, n_checks in {1, 5}, every optional array
    given or only the required ones: the staged extras are exactly the form's, with the sizes, flags and offsets of the rows each host form
    used to add by hand; way16 and wayq are the only inputs among them; pending is staged without an array of the caller's; after an early
    end `done` rows of every trace go back and everything else whole.  Block rows for k = 0, 1, 2 and the last k with and without q_traj,
    dist_traj, way_traj and io->goal_dist: block 0 reads io->q, the handle's q pair alternates, the *_prev rows are NULL at k = 0 and without
    a trace, a joint form never gets the handle's distance row."""
    assert "timed moves OK (576 cases)" in io_layout_output
