"""Host checks of the stages behind k_reconcile (isaac_ros_apriltag_amd/csrc/post_plan.h): what a setter's request makes of the
mode, when it retires the captured graphs, and what one submission launches there -- kernels, instances, record lists, grids and
the pinned blocks whose stamps the wait checks.  The expected plans are written out literally; the retirement rule is restated
here from the five setters' own conditions as they stood before the rule had one place."""
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# a mode: (nbundles, nrigid, iterations, sigma, nundist); the values of a stage that is on
NB, NR, IT, SG, NU = 2, 1, 5, 0.5, 2


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("post_plan") / "post_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(HERE, "aux_c", "post_plan_driver.cpp"), "-o", exe])

    def run(*words):
        out = subprocess.run([exe], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True, check=True).stdout
        return out.strip()
    return run


# ---- the plans -------------------------------------------------------------------------------------------------------------------------
# U k_undistort_records, P k_bundle_pose, R<cov> k_bundle_rigid<cov>, F<cov> k_pose_refine<cov>; r / t: the pose launch reads the raw
# records / the undistorted twins; gx x gy; > the pinned blocks it writes, /b<bundles> frames x bundles, /r<ostride> frames x records.
# Per reachable mode (planar and rigid are never both on): 3 frames at 64 record slots, then 1 frame at 1 slot.
PLANS = {
    # nothing on
    (0, 0, 0, 0, 0): ("", ""),
    (0, 0, 0, SG, 0): ("", ""),   # covariance alone: neither pose launch runs
    # refinement
    (0, 0, IT, 0, 0): ("F0r:3x8>rposes/r64", "F0r:1x1>rposes/r1"),
    (0, 0, IT, SG, 0): ("F1r:3x8>rposes/r64,rcovs/r64", "F1r:1x1>rposes/r1,rcovs/r1"),
    # planar bundles (k_bundle_pose has no covariance instance)
    (NB, 0, 0, 0, 0): ("Pr:3x8>bposes/b2", "Pr:1x8>bposes/b2"),
    (NB, 0, 0, SG, 0): ("Pr:3x8>bposes/b2", "Pr:1x8>bposes/b2"),
    (NB, 0, IT, 0, 0): ("Pr:3x8>bposes/b2 F0r:3x8>rposes/r64", "Pr:1x8>bposes/b2 F0r:1x1>rposes/r1"),
    (NB, 0, IT, SG, 0): ("Pr:3x8>bposes/b2 F1r:3x8>rposes/r64,rcovs/r64", "Pr:1x8>bposes/b2 F1r:1x1>rposes/r1,rcovs/r1"),
    # rigid bundles
    (0, NR, 0, 0, 0): ("R0r:3x8>xposes/b1", "R0r:1x8>xposes/b1"),
    (0, NR, 0, SG, 0): ("R1r:3x8>xposes/b1,xcovs/b1", "R1r:1x8>xposes/b1,xcovs/b1"),
    (0, NR, IT, 0, 0): ("R0r:3x8>xposes/b1 F0r:3x8>rposes/r64", "R0r:1x8>xposes/b1 F0r:1x1>rposes/r1"),
    (0, NR, IT, SG, 0): ("R1r:3x8>xposes/b1,xcovs/b1 F1r:3x8>rposes/r64,rcovs/r64", "R1r:1x8>xposes/b1,xcovs/b1 F1r:1x1>rposes/r1,rcovs/r1"),
    # the same twelve with the corner undistortion on: its launch first, and every pose launch on the twins
    (0, 0, 0, 0, NU): ("U:3x16>udets/r64", "U:1x16>udets/r1"),
    (0, 0, 0, SG, NU): ("U:3x16>udets/r64", "U:1x16>udets/r1"),
    (0, 0, IT, 0, NU): ("U:3x16>udets/r64 F0t:3x8>rposes/r64", "U:1x16>udets/r1 F0t:1x1>rposes/r1"),
    (0, 0, IT, SG, NU): ("U:3x16>udets/r64 F1t:3x8>rposes/r64,rcovs/r64", "U:1x16>udets/r1 F1t:1x1>rposes/r1,rcovs/r1"),
    (NB, 0, 0, 0, NU): ("U:3x16>udets/r64 Pt:3x8>bposes/b2", "U:1x16>udets/r1 Pt:1x8>bposes/b2"),
    (NB, 0, 0, SG, NU): ("U:3x16>udets/r64 Pt:3x8>bposes/b2", "U:1x16>udets/r1 Pt:1x8>bposes/b2"),
    (NB, 0, IT, 0, NU): ("U:3x16>udets/r64 Pt:3x8>bposes/b2 F0t:3x8>rposes/r64", "U:1x16>udets/r1 Pt:1x8>bposes/b2 F0t:1x1>rposes/r1"),
    (NB, 0, IT, SG, NU): ("U:3x16>udets/r64 Pt:3x8>bposes/b2 F1t:3x8>rposes/r64,rcovs/r64",
                          "U:1x16>udets/r1 Pt:1x8>bposes/b2 F1t:1x1>rposes/r1,rcovs/r1"),
    (0, NR, 0, 0, NU): ("U:3x16>udets/r64 R0t:3x8>xposes/b1", "U:1x16>udets/r1 R0t:1x8>xposes/b1"),
    (0, NR, 0, SG, NU): ("U:3x16>udets/r64 R1t:3x8>xposes/b1,xcovs/b1", "U:1x16>udets/r1 R1t:1x8>xposes/b1,xcovs/b1"),
    (0, NR, IT, 0, NU): ("U:3x16>udets/r64 R0t:3x8>xposes/b1 F0t:3x8>rposes/r64", "U:1x16>udets/r1 R0t:1x8>xposes/b1 F0t:1x1>rposes/r1"),
    (0, NR, IT, SG, NU): ("U:3x16>udets/r64 R1t:3x8>xposes/b1,xcovs/b1 F1t:3x8>rposes/r64,rcovs/r64",
                          "U:1x16>udets/r1 R1t:1x8>xposes/b1,xcovs/b1 F1t:1x1>rposes/r1,rcovs/r1"),
}
REACHABLE = sorted(PLANS)


def test_the_table_holds_every_reachable_mode():
    assert set(PLANS) == {(nb, nr, it, sg, nu) for nb, nr in ((0, 0), (NB, 0), (0, NR)) for it in (0, IT) for sg in (0, SG) for nu in (0, NU)}


@pytest.mark.parametrize("mode", REACHABLE)
def test_plan_of_each_reachable_mode(drv, mode):
    assert drv("plan", *mode, 3, 64) == PLANS[mode][0]
    assert drv("plan", *mode, 1, 1) == PLANS[mode][1]


def test_frames_and_stride_enter_separately(drv):
    """The other two pairings of the frame counts and strides, everything on: frames are the grids' first extent only, the stride
    is the record blocks' and the refinement's wave count (eight records per wave, at least one wave), bundles are neither."""
    assert drv("plan", NB, 0, IT, SG, NU, 1, 64) == "U:1x16>udets/r64 Pt:1x8>bposes/b2 F1t:1x8>rposes/r64,rcovs/r64"
    assert drv("plan", NB, 0, IT, SG, NU, 3, 1) == "U:3x16>udets/r1 Pt:3x8>bposes/b2 F1t:3x1>rposes/r1,rcovs/r1"
    assert drv("plan", 0, NR, IT, SG, NU, 1, 64) == "U:1x16>udets/r64 R1t:1x8>xposes/b1,xcovs/b1 F1t:1x8>rposes/r64,rcovs/r64"
    assert drv("plan", 0, NR, IT, SG, NU, 3, 1) == "U:3x16>udets/r1 R1t:3x8>xposes/b1,xcovs/b1 F1t:3x1>rposes/r1,rcovs/r1"
    assert drv("plan", 0, 8, IT, 0, 0, 3, 20) == "R0r:3x8>xposes/b8 F0r:3x3>rposes/r20"   # 20 slots: three waves; eight bundles


# ---- requests and retirement -----------------------------------------------------------------------------------------------------------
# every setter's request: off, the value of the modes above, another value
REQUESTS = [("planar", 0), ("planar", NB), ("planar", 3), ("rigid", 0), ("rigid", NR), ("rigid", 4), ("refine", 0), ("refine", IT),
            ("refine", 7), ("cov", 0), ("cov", SG), ("cov", 0.25), ("undistort", 0), ("undistort", NU), ("undistort", 1)]


def setters_as_they_were(mode, what, v):
    """(new mode, graphs retired): the five setters' own statements and drop_graphs conditions, each as its setter had it."""
    nb, nr, it, sg, nu = mode
    on = v > 0
    if what == "planar":      # amdAprilTagsSetBundles: on != (nbundles > 0) || (on && nrigid > 0); then nbundles = n, and nrigid = 0 if on
        return (v, 0 if on else nr, it, sg, nu), on != (nb > 0) or (on and nr > 0)
    if what == "rigid":       # amdAprilTagsSetBundlesEx: on != (nrigid > 0) || (on && nbundles > 0); then nrigid = n, and nbundles = 0 if on
        return (0 if on else nb, v, it, sg, nu), on != (nr > 0) or (on and nb > 0)
    if what == "refine":      # amdAprilTagsSetPoseRefinement: on != (pose_iterations > 0)
        return (nb, nr, v, sg, nu), on != (it > 0)
    if what == "cov":         # amdAprilTagsSetPoseCovariance: on != (pose_cov_sigma > 0.0)
        return (nb, nr, it, v, nu), on != (sg > 0)
    return (nb, nr, it, sg, v), on != (nu > 0)   # amdAprilTagsSetCornerUndistortion: on != !undist_models.empty()


def apply(drv, mode, what, v):
    new, keys = drv("apply", *mode, what, v).split("|")
    nb, nr, it, sg, nu = new.split()
    before, after, retired = map(int, keys.split())
    assert retired == int(before != after)
    return (int(nb), int(nr), int(it), float(sg), int(nu)), bool(retired)


@pytest.mark.parametrize("what,v", REQUESTS)
def test_every_request_on_every_reachable_mode(drv, what, v):
    for mode in REACHABLE:
        new, retired = apply(drv, mode, what, v)
        want, want_retired = setters_as_they_were(mode, what, v)
        assert (new, retired) == (want, want_retired), (mode, what, v)
        assert not (new[0] and new[1]), "planar and rigid both on"


def test_named_cases(drv):
    # covariance toggled with no pose launch on: the graphs are retired all the same, in both directions
    assert apply(drv, (0, 0, 0, 0, 0), "cov", SG) == ((0, 0, 0, SG, 0), True)
    assert apply(drv, (0, 0, 0, SG, 0), "cov", 0) == ((0, 0, 0, 0, 0), True)
    assert apply(drv, (NB, 0, 0, 0, NU), "cov", SG) == ((NB, 0, 0, SG, NU), True)   # (k_bundle_pose has no covariance instance)
    # same bits, another value: nothing is retired
    assert apply(drv, (NB, 0, IT, SG, NU), "planar", 3) == ((3, 0, IT, SG, NU), False)
    assert apply(drv, (0, NR, IT, SG, NU), "rigid", 4) == ((0, 4, IT, SG, NU), False)
    assert apply(drv, (NB, 0, IT, SG, NU), "refine", 7) == ((NB, 0, 7, SG, NU), False)
    assert apply(drv, (NB, 0, IT, SG, NU), "cov", 0.25) == ((NB, 0, IT, 0.25, NU), False)
    assert apply(drv, (NB, 0, IT, SG, NU), "undistort", 1) == ((NB, 0, IT, SG, 1), False)
    # one kind on turns the other off, once; off leaves the other alone and retires nothing where it was off already
    assert apply(drv, (NB, 0, 0, 0, 0), "rigid", NR) == ((0, NR, 0, 0, 0), True)
    assert apply(drv, (0, NR, 0, 0, 0), "planar", NB) == ((NB, 0, 0, 0, 0), True)
    assert apply(drv, (NB, 0, 0, 0, 0), "rigid", 0) == ((NB, 0, 0, 0, 0), False)
    assert apply(drv, (0, NR, 0, 0, 0), "planar", 0) == ((0, NR, 0, 0, 0), False)


def test_the_key_is_the_five_bits(drv):
    """undistort 1, planar 2, rigid 4, refine 8, covariance 16: distinct for the 24 reachable modes."""
    keys = {mode: int(drv("apply", *mode, "refine", mode[2]).split("|")[1].split()[0]) for mode in REACHABLE}
    assert keys[(NB, 0, IT, SG, NU)] == 1 + 2 + 8 + 16 and keys[(0, NR, 0, 0, 0)] == 4 and keys[(0, 0, 0, SG, 0)] == 16
    assert len(set(keys.values())) == len(REACHABLE) == 24
    assert all(itertools.starmap(lambda m, k: bool(k & 2) == (m[0] > 0) and bool(k & 4) == (m[1] > 0), keys.items()))
