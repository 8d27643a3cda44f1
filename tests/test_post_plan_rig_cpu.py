"""Host checks of the camera rig's row in the stages behind k_reconcile (isaac_ros_apriltag_amd/csrc/post_plan.h): the plans of the
rig-on modes written out literally, that the rig changes nothing where the rigid kind is off, the request and the sixth key bit.
tests/test_post_plan_cpu.py holds the rig-off modes, which stay what they were."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# a mode: (nbundles, nrigid, iterations, sigma, nundist, nrig); the values of a stage that is on
NB, NR, IT, SG, NU, NG = 2, 1, 5, 0.5, 2, 3


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("post_plan_rig") / "post_plan_rig_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(HERE, "aux_c", "post_plan_rig_driver.cpp"), "-o", exe])

    def run(*words):
        return subprocess.run([exe], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True, check=True).stdout.strip()
    return run


# G k_bundle_rig: behind every other pose launch, grid frames x AMDAT_MAX_BUNDLES, one block gposes of groups x bundles (a group index
# per frame), raw records or twins as the other pose launches, never a covariance.  3 frames at 64 record slots, then 1 frame at 1 slot.
PLANS = {
    (0, NR, 0, 0, 0, NG): ("R0r:3x8>xposes/b1 Gr:3x8>gposes/b1", "R0r:1x8>xposes/b1 Gr:1x8>gposes/b1"),
    (0, NR, 0, SG, 0, NG): ("R1r:3x8>xposes/b1,xcovs/b1 Gr:3x8>gposes/b1", "R1r:1x8>xposes/b1,xcovs/b1 Gr:1x8>gposes/b1"),
    (0, NR, IT, 0, 0, NG): ("R0r:3x8>xposes/b1 F0r:3x8>rposes/r64 Gr:3x8>gposes/b1", "R0r:1x8>xposes/b1 F0r:1x1>rposes/r1 Gr:1x8>gposes/b1"),
    (0, NR, IT, SG, 0, NG): ("R1r:3x8>xposes/b1,xcovs/b1 F1r:3x8>rposes/r64,rcovs/r64 Gr:3x8>gposes/b1",
                             "R1r:1x8>xposes/b1,xcovs/b1 F1r:1x1>rposes/r1,rcovs/r1 Gr:1x8>gposes/b1"),
    (0, NR, 0, 0, NU, NG): ("U:3x16>udets/r64 R0t:3x8>xposes/b1 Gt:3x8>gposes/b1", "U:1x16>udets/r1 R0t:1x8>xposes/b1 Gt:1x8>gposes/b1"),
    (0, NR, 0, SG, NU, NG): ("U:3x16>udets/r64 R1t:3x8>xposes/b1,xcovs/b1 Gt:3x8>gposes/b1",
                             "U:1x16>udets/r1 R1t:1x8>xposes/b1,xcovs/b1 Gt:1x8>gposes/b1"),
    (0, NR, IT, 0, NU, NG): ("U:3x16>udets/r64 R0t:3x8>xposes/b1 F0t:3x8>rposes/r64 Gt:3x8>gposes/b1",
                             "U:1x16>udets/r1 R0t:1x8>xposes/b1 F0t:1x1>rposes/r1 Gt:1x8>gposes/b1"),
    (0, NR, IT, SG, NU, NG): ("U:3x16>udets/r64 R1t:3x8>xposes/b1,xcovs/b1 F1t:3x8>rposes/r64,rcovs/r64 Gt:3x8>gposes/b1",
                              "U:1x16>udets/r1 R1t:1x8>xposes/b1,xcovs/b1 F1t:1x1>rposes/r1,rcovs/r1 Gt:1x8>gposes/b1"),
}


@pytest.mark.parametrize("mode", sorted(PLANS))
def test_plan_of_each_rig_mode(drv, mode):
    assert drv("plan", *mode, 3, 64) == PLANS[mode][0]
    assert drv("plan", *mode, 1, 1) == PLANS[mode][1]


def test_the_block_follows_the_rigid_count_not_the_cameras(drv):
    assert drv("plan", 0, 8, 0, 0, 0, 16, 4, 20) == "R0r:4x8>xposes/b8 Gr:4x8>gposes/b8"
    assert drv("plan", 0, 8, 0, 0, 0, 1, 4, 20) == "R0r:4x8>xposes/b8 Gr:4x8>gposes/b8"


@pytest.mark.parametrize("nb,nr", ((0, 0), (NB, 0)))
@pytest.mark.parametrize("it", (0, IT))
@pytest.mark.parametrize("sg", (0, SG))
@pytest.mark.parametrize("nu", (0, NU))
def test_without_the_rigid_kind_the_rig_launches_nothing(drv, nb, nr, it, sg, nu):
    for n, ostride in ((3, 64), (1, 1)):
        assert drv("plan", nb, nr, it, sg, nu, NG, n, ostride) == drv("plan", nb, nr, it, sg, nu, 0, n, ostride)
        assert "G" not in drv("plan", nb, nr, it, sg, nu, NG, n, ostride)


def apply(drv, mode, what, v):
    new, keys = drv("apply", *mode, what, v).split("|")
    nb, nr, it, sg, nu, ng = new.split()
    before, after, retired = map(int, keys.split())
    assert retired == int(before != after)
    return (int(nb), int(nr), int(it), float(sg), int(nu), int(ng)), before, after, bool(retired)


def test_the_request_and_the_sixth_bit(drv):
    # on and off retire, whatever else is on -- also with the rigid kind off, where nothing is launched; another count does not
    for base in ((0, 0, 0, 0, 0), (0, NR, 0, 0, 0), (NB, 0, IT, SG, NU), (0, NR, IT, SG, NU)):
        new, before, after, retired = apply(drv, base + (0,), "rig", NG)
        assert new == base + (NG,) and after == before + 32 and retired
        new, before, after, retired = apply(drv, base + (NG,), "rig", 0)
        assert new == base + (0,) and after == before - 32 and retired
        new, before, after, retired = apply(drv, base + (NG,), "rig", 2)
        assert new == base + (2,) and after == before and not retired
        assert apply(drv, base + (0,), "rig", 0) == (base + (0,), before - 32, before - 32, False)
    # the other setters leave the rig alone, and it leaves them alone
    assert apply(drv, (NB, 0, 0, 0, 0, NG), "rigid", NR)[0] == (0, NR, 0, 0, 0, NG)
    assert apply(drv, (0, NR, 0, 0, 0, NG), "rigid", 0)[0] == (0, 0, 0, 0, 0, NG)
    assert apply(drv, (0, NR, 0, 0, 0, NG), "planar", NB)[0] == (NB, 0, 0, 0, 0, NG)
    assert apply(drv, (0, NR, IT, SG, NU, NG), "cov", 0)[0] == (0, NR, IT, 0, NU, NG)
    # with the rig off every key is the five bits it was
    assert apply(drv, (NB, 0, IT, SG, NU, 0), "refine", IT)[1] == 1 + 2 + 8 + 16
    assert apply(drv, (0, NR, IT, SG, NU, NG), "refine", IT)[1] == 1 + 4 + 8 + 16 + 32
