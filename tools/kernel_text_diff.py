#!/usr/bin/env python3
"""Compare the gfx950 device code of two checkouts kernel by kernel:  python tools/kernel_text_diff.py <tree A> <tree B>

Every file of each tree's _lib.SOURCES is compiled to assembly text with that tree's _lib.HIPCC_FLAGS (no GPU needed).  Per kernel
symbol two things are compared: the instruction lines (comments stripped, the numbers of local .LBB / .Ltmp labels normalised)
and the .amdhsa_* lines of the kernel descriptor (registers, LDS, scratch).  Prints a markdown table `kernel, unit in A, unit in
B, lines, SAME/DIFF`; exits non-zero on any DIFF or on a kernel that only one side has.  A refactor that moves kernels between
units or shares helpers between them is safe for speed exactly when every row says SAME (profiles/kernel_units_isa.md).
"""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def kernels_of(tree, tmp):
    """{kernel symbol: (unit, instruction lines, descriptor lines)} of one checkout"""
    spec = importlib.util.spec_from_file_location("_lib_of_tree", os.path.join(tree, "thr3ed_atom_amd", "_lib.py"))
    lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib)
    flags = [f for f in lib.HIPCC_FLAGS if f != "-shared"] + ["--cuda-device-only", "-S", "-I", lib.INCLUDE_DIR]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def compile_unit(unit):
        out = os.path.join(tmp, unit + ".s")
        done = subprocess.run([hipcc] + flags + [os.path.join(lib.CSRC_DIR, unit), "-o", out], stderr=subprocess.PIPE, text=True)
        # (hipcc's one standing remark about the unused --hip-link is dropped; every other diagnostic is passed on)
        noise = [l for l in done.stderr.splitlines() if l.strip() and "argument unused during compilation: '--hip-link'" not in l]
        if noise:
            print(f"{tree}: {unit}:\n" + "\n".join(noise), file=sys.stderr)
        if done.returncode:
            sys.exit(f"{tree}: {unit} does not compile")
        return open(out).read()

    found = {}
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for unit, text in zip(lib.SOURCES, pool.map(compile_unit, lib.SOURCES)):
            for name, desc in re.findall(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
                body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S).group(1)
                lines = [re.sub(r"\.(LBB|Ltmp)\d+", r".\1", line.split(";")[0]).strip() for line in body.split("\n")]
                found[name] = (unit, [l for l in lines if l], [l.strip() for l in desc.split("\n") if l.strip()])
    return found


def main(tree_a, tree_b):
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a, b = kernels_of(os.path.abspath(tree_a), ta), kernels_of(os.path.abspath(tree_b), tb)
    print("| kernel | unit in A | unit in B | lines | |\n|---|---|---|---|---|")
    bad = 0
    for name in sorted(set(a) | set(b)):
        ua, ia, da = a.get(name, ("-", None, None))
        ub, ib, db = b.get(name, ("-", None, None))
        same = ia is not None and ia == ib and da == db
        bad += not same
        print(f"| `{name}` | {ua} | {ub} | {len(ib if ib is not None else ia)} | {'SAME' if same else 'DIFF'} |")
    print(f"\n{len(a)} kernels in A, {len(b)} in B, {bad} differ or are missing on one side.")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
