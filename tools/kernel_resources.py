#!/usr/bin/env python3
"""Prints VGPR / spill / LDS / occupancy of every kernel of the library (hipcc -Rpass-analysis=kernel-resource-usage).
Usage: python tools/kernel_resources.py [extra hipcc flags]    compiles detector.hip again with those flags and reports
       python tools/kernel_resources.py --built                reports what the product build wrote beside libapriltag_amd.so"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaac_ros_apriltag_amd import build as b   # the remarks' parser is the build's (build.resource_remarks / parse_resources)

if sys.argv[1:] == ["--built"]:
    with open(b.RESOURCES_AMD) as f:
        text, rest = f.read(), ""
else:
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
               "-Rpass-analysis=kernel-resource-usage", os.path.join(ROOT, "isaac_ros_apriltag_amd", "csrc", "detector.hip"),
               "-o", os.path.join(tmp, "_res.so")] + sys.argv[1:]
        text, rest = b.resource_remarks(subprocess.run(cmd, capture_output=True, text=True).stderr)
print("%-36s %6s %6s %8s %8s %6s %8s" % ("kernel", "VGPR", "AGPR", "spillV", "scratch", "occ", "LDS"))
for k, r in b.parse_resources(text).items():
    print("%-36s %6d %6d %8d %8d %6d %8d" % (k[:36], r.get("VGPRs", 0), r.get("AGPRs", 0), r.get("VGPRs Spill", r.get("VGPR Spill", 0)),
                                          r.get("ScratchSize", 0), r.get("Occupancy", 0), r.get("LDS Size", 0)))
if "error" in rest:
    print(rest[-3000:])
