"""The staging layout of the host-pointer call forms (vfclik_amd/csrc/vfik_io_layout.h): tests/c_host/io_layout.cpp -- host code
only, no HIP, no library -- under AddressSanitizer + UBSan, as a process of its own.  For 6 / 7 / 16 joints, both element sizes,
1 / 37 / 700 arms and three member subsets (q and qdot_out; everything; everything plus a goto's four extras) it checks that every
present member is 256-byte aligned, that no two overlap, that the inputs are a prefix, that absent members take no room and that
the total is the sum of the rounded sizes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_io_layout_under_asan_ubsan(tmp_path):
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
    assert "io_layout OK (54 cases)" in r.stdout
