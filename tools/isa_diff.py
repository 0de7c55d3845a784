#!/usr/bin/env python
"""Compare the gfx950 device code of two builds, kernel by kernel: what decides whether a refactor left the kernels alone.
python tools/isa_diff.py A B -- two directories of built objects (csrc/ after make), or two libvfik_hip.so.
Per object: kernels only in A, only in B, how many are identical, and both instruction counts of each that differs; likewise the
resource remarks (<object>.resusage.txt) where they lie beside the objects.  Exit status 1 when a kernel present in both differs.
It compares instruction text (addresses and encodings dropped, branch targets kept as their relative offsets); it needs no GPU."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
PRETTY = {}   # mangled symbol -> demangled, as llvm-objdump writes it


def kernels(path):
    """{mangled symbol: [instruction, ...]} over the gfx950 code objects bundled in an object file or a shared library"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(path, os.path.join(d, "x"))
        subprocess.run([OBJDUMP, "--offloading", "x"], cwd=d, check=True, capture_output=True)
        for co in sorted(glob.glob(os.path.join(d, "x.*gfx950"))):
            run = lambda *opt: subprocess.run([OBJDUMP, *opt, co], check=True, capture_output=True, text=True).stdout
            txt = run("-d")
            # "0000000000019300 g     F .text\t00000000000029d4 .protected <name>", the same lines with and without -C
            name = lambda ln: re.sub(r"^\S+ (\.\w+ )?", "", ln.split(".text\t", 1)[1])
            PRETTY.update((name(m), name(p)) for m, p in zip(run("--syms").split("\n"), run("--syms", "-C").split("\n")) if " F .text" in m)
            for block in re.split(r"\n(?=[0-9a-f]{16} <)", txt)[1:]:
                head, *lines = block.split("\n")
                # "\ts_branch 56   // 00000001931C: BF820038 <sym+0x100>": the text in front of the comment is the instruction
                out[head[18:-2]] = [ln.split("//")[0].strip() for ln in lines if ln.startswith("\t")]
    return out


def remarks(path):
    """{mangled symbol: [remark, ...]} of a -Rpass-analysis=kernel-resource-usage log, or None without one"""
    if not os.path.exists(path):
        return None
    out, cur = {}, None
    for m in re.finditer(r"remark:\s+(.*?) \[-Rpass-analysis", open(path).read()):
        if m.group(1).startswith("Function Name: "):
            cur = out.setdefault(m.group(1)[15:], [])
        elif cur is not None:
            cur.append(m.group(1))
    return out


def demangle(names):
    return [PRETTY.get(n, n) for n in names]


def main():
    a, b = sys.argv[1:3]
    if os.path.isdir(a):
        pairs = [(os.path.basename(p), p, os.path.join(b, os.path.basename(p))) for p in sorted(glob.glob(os.path.join(a, "*.o")))]
    else:
        pairs = [(os.path.basename(a), a, b)]
    differ = 0
    for name, pa, pb in pairs:
        ka, kb = kernels(pa), kernels(pb)
        if not ka and not kb:
            continue   # host code only
        ra, rb = (remarks(os.path.splitext(p)[0] + ".resusage.txt") for p in (pa, pb))
        both = [k for k in ka if k in kb]
        diff = [k for k in both if ka[k] != kb[k]]
        rdiff = [k for k in both if ra is not None and rb is not None and ra.get(k) != rb.get(k)]
        print("%s: %d kernels in A, %d in B; %d identical, %d differ; resource remarks: %s" % (
            name, len(ka), len(kb), len(both) - len(diff), len(diff),
            "none beside the objects" if ra is None or rb is None else "%d identical, %d differ" % (len(both) - len(rdiff), len(rdiff))))
        for k in demangle([k for k in ka if k not in kb]):
            print("  only in A: " + k)
        for k in demangle([k for k in kb if k not in ka]):
            print("  only in B: " + k)
        for k, n in zip(diff, demangle(diff)):
            print("  differs (%d / %d instructions): %s" % (len(ka[k]), len(kb[k]), n))
        for k, n in zip(rdiff, demangle(rdiff)):
            print("  remarks differ: %s\n    A: %s\n    B: %s" % (n, "; ".join(ra.get(k, [])), "; ".join(rb.get(k, []))))
        differ += len(diff) + len(rdiff)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
