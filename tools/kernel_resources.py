#!/usr/bin/env python
"""Per-kernel register / LDS / occupancy summary of HIP sources (hipcc -Rpass-analysis=kernel-resource-usage).
usage: python tools/kernel_resources.py [file.hip] [include dir] [substring filter ...]
Without a file (or with "-" in its place) every unit of thr3ed_atom_amd/_lib.py:SOURCES is covered."""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thr3ed_atom_amd import _lib  # noqa: E402  (ctypes only: nothing is loaded)

srcs = [sys.argv[1]] if len(sys.argv) > 1 and sys.argv[1] != "-" else [os.path.join(_lib.CSRC_DIR, s) for s in _lib.SOURCES]
inc = sys.argv[2] if len(sys.argv) > 2 else _lib.INCLUDE_DIR
filters = sys.argv[3:]
cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", inc, *srcs, "-o", "/tmp/kr.so",
       "-Rpass-analysis=kernel-resource-usage"]
out = subprocess.run(cmd, capture_output=True, text=True).stderr
cur, rows = None, {}
keys = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")
for line in out.splitlines():
    if " error" in line:
        print(line)
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        cur = re.sub(r"\(anonymous namespace\)::", "", cur)
        cur = re.sub(r"\(.*", "", cur).replace("void ", "")
        rows[cur] = {}
        continue
    for k in keys:
        m = re.search(re.escape(k) + r": (\d+)", line)
        if m and cur and k not in rows[cur]:
            rows[cur][k] = int(m.group(1))
for k, v in rows.items():
    if filters and not any(f in k for f in filters):
        continue
    g = lambda n: v.get(n, 0)
    print(f"{k:52s} vgpr {g('VGPRs'):4d} agpr {g('AGPRs'):3d} scratch {g('ScratchSize [bytes/lane]'):4d} occ {g('Occupancy [waves/SIMD]')} sgpr-spill {g('SGPRs Spill'):3d} vgpr-spill {g('VGPRs Spill'):3d} lds {g('LDS Size [bytes/block]')}")
