"""Kernels of the timed path that must need no private segment (scratch), read from what the product build wrote beside
libapriltag_amd.so (isaac_ros_apriltag_amd/build.py: the kernel-resource-usage remarks of that very compile; nothing is compiled
here).  No result depends on it, only the speed: in the first submission of a process a k_fit_quads launch whose instance needs
scratch starts 0.13 ms behind its predecessor on the submission stream, the instances without are 0.1 ms of the fit stage faster
in every step, and a few spilled loop invariants are enough to need a private segment -- the
spills came back twice unnoticed.  k_decode_wave is not in the list: it went from 36 to 6 spilled registers, and no form that was
tried reaches none at its 80 registers."""
import os
import re

import pytest

from isaac_ros_apriltag_amd import build as b

# every instance the library holds of these kernels (templates: all instantiations)
SCRATCH_FREE = ("k_fit_quads", "k_fit_small", "k_fit_prefilter", "k_points", "k_scatter", "k_cc_local", "k_threshold")
# instances that have to be there, so that a renamed kernel cannot empty the check
INSTANCES = tuple("k_fit_quads<%d, %s>" % (nt, s) for s in ("true", "false") for nt in (64, 128, 256, 512, 1024)) + (
    "k_fit_small<2>", "k_fit_prefilter<64>", "k_fit_prefilter<1024>", "k_points", "k_scatter", "k_cc_local<4>", "k_cc_local<16>")


@pytest.fixture(scope="module")
def rows():
    assert os.path.exists(b.RESOURCES_AMD), "%s is missing: written by isaac_ros_apriltag_amd.build.build_amd()" % b.RESOURCES_AMD
    with open(b.RESOURCES_AMD) as f:
        return b.parse_resources(f.read())


def base(name):
    return re.sub(r"<.*", "", name)


def test_file_belongs_to_the_library(rows):
    assert os.path.exists(b.LIB_AMD)
    assert len(rows) > 40 and all("ScratchSize" in r and "VGPRs" in r for r in rows.values())


def test_listed_instances_are_present(rows):
    assert not [n for n in INSTANCES if n not in rows]
    assert any(base(n) == "k_threshold" for n in rows)


def test_no_private_segment(rows):
    bad = {n: (r["ScratchSize"], r.get("VGPRs Spill")) for n, r in rows.items()
           if base(n) in SCRATCH_FREE and (r["ScratchSize"] != 0 or r.get("VGPRs Spill", 0) != 0)}
    assert not bad, "ScratchSize [bytes/lane], spilled VGPRs: %s" % bad


def test_fit_occupancy(rows):
    """4 waves per SIMD for every fit kernel (FQ_WPE_*, FS_WPE, the prefilter's register use): the budget the spills must not buy."""
    low = {n: r["Occupancy"] for n, r in rows.items() if base(n) in ("k_fit_quads", "k_fit_small", "k_fit_prefilter") and r["Occupancy"] < 4}
    assert not low, low
