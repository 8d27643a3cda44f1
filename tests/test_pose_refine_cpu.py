"""CPU checks of the orthogonal-iteration tag pose with both minima (amdAprilTagsSetPoseRefinement): the Python
reference tests/pose_refine_ref.py against analytic truth, its benefit over the homography pose on a seeded noisy set, a constructed
case of the planar ambiguity, the header csrc/pose_refine.h compiled by g++ against the reference bit for bit (also under the host
sanitizers in a program of its own), the oracle-side preconditions of the GPU test, and the ABI."""
import ctypes as C
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from isaac_ros_apriltag_amd import build, capi  # noqa: E402
import bundle_cases as bc  # noqa: E402
import pose_refine_cases as pc  # noqa: E402
import pose_refine_ref as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "aux_c", "pose_refine_driver.cpp")
INVALID_ARGUMENT = 1
INTR = (600.0, 600.0, 320.0, 240.0)
SIZE = float(np.float32(0.1))   # a tag_size the C ABI carries exactly (f32)
_cache = {}


def _truth_cases():
    """50 seeded poses, tilt up to 70 degrees, a skew on every third: (corners, intrinsics, skew, R, t, R_h, t_h)."""
    if "truth" not in _cache:
        rng = np.random.default_rng(50)
        out = []
        for i in range(50):
            R, t = pc.random_pose(rng, 0.0, 70.0)
            skew = 0.75 if i % 3 == 1 else 0.0
            p = pc.project(R, t, INTR, skew, SIZE)
            Rh, th = pc.homography_pose(p, INTR, skew, SIZE)
            out.append((p, INTR, skew, R, t, Rh, th))
        _cache["truth"] = out
    return _cache["truth"]


def _noisy_cases():
    """400 seeded poses (0.1 m tag at 0.6 .. 1.2 m, 20 .. 60 degrees of tilt, f = 600 px), Gaussian corner noise of 0.3 px."""
    if "noisy" not in _cache:
        rng = np.random.default_rng(7)
        out = []
        for _ in range(400):
            R, t = pc.random_pose(rng, 20.0, 60.0)
            p = pc.project(R, t, INTR, 0.0, SIZE) + rng.normal(0.0, 0.3, (4, 2))
            Rh, th = pc.homography_pose(p, INTR, 0.0, SIZE)
            out.append((p, INTR, 0.0, R, t, Rh, th))
        _cache["noisy"] = out
    return _cache["noisy"]


def _noisy_refined():
    if "noisy_ref" not in _cache:
        _cache["noisy_ref"] = [pr.refine(p, intr, skew, SIZE, Rh, th, pc.ITERATIONS) for (p, intr, skew, _, _, Rh, th) in _noisy_cases()]
    return _cache["noisy_ref"]


def _ambiguous_case():
    """A small tag far away and a little noise, handed over with the WRONG minimum as its homography pose: the alternative of a first
    run (from the true side) is the start, so chain 0 stays in the wrong basin and the mirrored chain finds the better pose."""
    if "ambiguous" not in _cache:
        rng = np.random.default_rng(3)
        R = pc.rodrigues((math.cos(0.4), math.sin(0.4), 0.0), math.radians(40.0))
        t = np.array([0.05, -0.03, 1.0])
        p = pc.project(R, t, INTR, 0.0, SIZE) + rng.normal(0.0, 0.1, (4, 2))
        Rh, th = pc.homography_pose(p, INTR, 0.0, SIZE)
        first = pr.refine(p, INTR, 0.0, SIZE, Rh, th, pc.ITERATIONS)
        _cache["ambiguous"] = (p, INTR, 0.0, R, t, first["R_alt"], first["t_alt"], first)
    return _cache["ambiguous"]


# ---- the reference -------------------------------------------------------------------------------------------------------------------------
def test_reference_against_truth(built):
    """Exact corners: the chosen pose is the truth.  E at rounding level: the corners carry at most an ulp of 640 px (2^-43) over
    f = 600 px, a ray error of 2e-16 at up to 1.3 m, and the statements between them and E a few hundred roundings of quantities of
    order one -- residuals of order 1e3 * 2^-53 m at the very most, E <= 4 (1.2e-13)^2 < 1e-24 m^2."""
    worst_e, worst_a = 0.0, 0.0
    for (p, intr, skew, R, t, Rh, th) in _truth_cases():
        out = pr.refine(p, intr, skew, SIZE, Rh, th, pc.ITERATIONS)
        assert out["status"] == pr.REFINED
        worst_e = max(worst_e, out["err"])
        worst_a = max(worst_a, pr.rot_angle_deg(out["R"], R))
        assert np.abs(out["t"] - t).max() < 1e-7
    print("truth: largest E %.3g m^2, largest rotation error %.3g degrees" % (worst_e, worst_a))
    assert worst_e < 1e-24 and worst_a < 1e-6


def test_benefit_over_the_homography_pose(built):
    """The condition of the feature: on the seeded noisy set the median rotation error of the chosen pose is at most half the
    homography pose's, err <= err_homography for every case, and every case is REFINED."""
    cases, ref = _noisy_cases(), _noisy_refined()
    eh = [pr.rot_angle_deg(Rh, R) for (_, _, _, R, _, Rh, _) in cases]
    er = [pr.rot_angle_deg(o["R"], R) for o, (_, _, _, R, _, _, _) in zip(ref, cases)]
    print("rotation error in degrees, homography pose / chosen pose: median %.3f / %.3f, 95th percentile %.2f / %.2f, above 10: %d / %d; "
          "chain 1 chosen in %d of %d" % (np.median(eh), np.median(er), np.percentile(eh, 95), np.percentile(er, 95), sum(e > 10 for e in eh),
                                          sum(e > 10 for e in er), sum(o["chosen"] for o in ref), len(ref)))
    assert all(o["status"] == pr.REFINED for o in ref)
    assert all(o["err"] <= o["err_homography"] for o in ref)
    assert np.median(er) <= 0.5 * np.median(eh)
    # the two chains end in distinct minima
    assert all(pr.rot_angle_deg(o["R"], o["R_alt"]) > 1.0 for o in ref)


def test_ambiguity_chain_1_chosen(built):
    p, intr, skew, R, t, Rh, th, first = _ambiguous_case()
    out = pr.refine(p, intr, skew, SIZE, Rh, th, pc.ITERATIONS)
    print("ambiguity: from the wrong side chosen %d, err %.3g against %.3g; %.3f degrees from the truth, the alternative %.2f"
          % (out["chosen"], out["err"], out["err_alt"], pr.rot_angle_deg(out["R"], R), pr.rot_angle_deg(out["R_alt"], R)))
    assert first["status"] == pr.REFINED and first["chosen"] == 0 and pr.rot_angle_deg(first["R"], first["R_alt"]) > 10.0
    assert out["status"] == pr.REFINED and out["chosen"] == 1 and out["err"] < out["err_alt"]
    assert pr.rot_angle_deg(out["R"], R) < 2.0 and pr.rot_angle_deg(out["R_alt"], R) > 10.0
    # the same two minima, whichever side the start is on
    assert pr.rot_angle_deg(out["R"], first["R"]) < 1e-3 and pr.rot_angle_deg(out["R_alt"], first["R_alt"]) < 1e-3


def test_gpu_preconditions_on_the_oracle_side(built):
    """What tests/test_pose_refine_gpu.py relies on: the oblique frame's four tags are found, refined, and their two minima differ; the
    wrong builds' forms of the definition give other records; hooks 17 and 18 are registered."""
    recs = pc.oblique_records()
    assert [r["id"] for r in recs] == sorted(o[0] for o in pc.OBLIQUE)
    ref = pc.refined("oblique", recs, pc.INTR_O, 0.0, pc.SIZE_O)
    for r, o in zip(recs, ref):
        i = [k for k, x in enumerate(pc.OBLIQUE) if x[0] == r["id"]][0]
        R, _ = pc.oblique_pose(i)
        assert o["status"] == pr.REFINED and pr.rot_angle_deg(o["R"], o["R_alt"]) > 20.0 and o["err"] < o["err_alt"]
        assert pr.rot_angle_deg(o["R"], R) <= pr.rot_angle_deg(r["R"], R)   # no further from the truth than the homography pose
    assert len(bc.records72()) == 72
    all_six = pc.content_refined("all_six")
    slot = bc.SLOTS["all_six"][1]
    args = (bc.content_records("all_six"), bc.INTR1[slot], bc.SKEW1[slot], bc.SIZE1, pc.ITERATIONS)
    unmirrored = pr.refine_records(*args, mirrored=False)
    stale_t = pr.refine_records(*args, t_follows_step=lambda it, n: it + 1 < n)
    assert all(pr.compare(a, b) for a, b in zip(unmirrored, all_six)) and all(pr.compare(a, b) for a, b in zip(stale_t, all_six))
    assert pc.content_refined("no_tags") == []
    hooks = open(os.path.join(ROOT, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    assert 17 in build.MUTANTS and 18 in build.MUTANTS and "AMDAT_MUTATE == 17" in hooks and "AMDAT_MUTATE == 18" in hooks


# ---- the header ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pose_refine") / "libpose_refine.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", DRIVER, "-o", so])
    L = C.CDLL(so)
    L.pose_refine_probe.argtypes = [C.POINTER(C.c_double)] + [C.c_double] * 6 + [C.POINTER(C.c_double)] * 2 + [C.c_uint32, C.POINTER(capi.RefinedPose)]
    L.pose_refine_probe.restype = None
    L.pose_refine_sizes.restype = C.c_uint32

    def probe(p, intr, skew, size, Rh, th, iterations):
        o = capi.RefinedPose()
        p8 = (C.c_double * 8)(*[float(v) for pt in p for v in pt])
        L.pose_refine_probe(p8, *[pr.f32(v) for v in intr], pr.f32(skew), pr.f32(size), (C.c_double * 9)(*np.asarray(Rh, dtype=np.float64).reshape(-1)),
                            (C.c_double * 3)(*np.asarray(th, dtype=np.float64).reshape(-1)), iterations, C.byref(o))
        return {"status": int(o.status), "chosen": int(o.chosen), "R": np.array(list(o.R)).reshape(3, 3), "t": np.array(list(o.t)), "err": float(o.err),
                "R_alt": np.array(list(o.R_alt)).reshape(3, 3), "t_alt": np.array(list(o.t_alt)), "err_alt": float(o.err_alt),
                "err_homography": float(o.err_homography)}
    probe.lib = L
    return probe


def test_header_equals_the_reference(built, header):
    """csrc/pose_refine.h under g++ against the Python reference, every field bit for bit: the truth cases (skew among them), the
    noisy set, the ambiguity case, the counts 1 and 200, and the degenerate record of four equal corners."""
    errs = []
    for i, (p, intr, skew, _, _, Rh, th) in enumerate(_truth_cases()):
        errs += pr.compare(header(p, intr, skew, SIZE, Rh, th, pc.ITERATIONS), pr.refine(p, intr, skew, SIZE, Rh, th, pc.ITERATIONS), "truth %d: " % i)
    for i, ((p, intr, skew, _, _, Rh, th), want) in enumerate(zip(_noisy_cases(), _noisy_refined())):
        errs += pr.compare(header(p, intr, skew, SIZE, Rh, th, pc.ITERATIONS), want, "noisy %d: " % i)
    p, intr, skew, _, _, Rh, th, _ = _ambiguous_case()
    for it in (1, 2, pc.ITERATIONS, 200):
        got = header(p, intr, skew, SIZE, Rh, th, it)
        errs += pr.compare(got, pr.refine(p, intr, skew, SIZE, Rh, th, it), "ambiguous, %d iterations: " % it)
    assert got["chosen"] == 1
    same = np.full((4, 2), 100.0)
    got, want = header(same, INTR, 0.0, SIZE, Rh, th, pc.ITERATIONS), pr.refine(same, INTR, 0.0, SIZE, Rh, th, pc.ITERATIONS)
    errs += pr.compare(got, want, "equal corners: ")
    assert want["status"] == pr.DEGENERATE and want["chosen"] == 0 and np.array_equal(want["R"], np.asarray(Rh).reshape(3, 3))
    assert not want["R_alt"].any() and not want["t_alt"].any() and want["err_alt"] == 0.0 and want["err"] == want["err_homography"]
    print(errs[:10])
    assert not errs


def test_header_under_asan_ubsan(tmp_path):
    """The same header in a program of its own (the driver's main), built with -fsanitize=address,undefined and run here."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void){return 0;}\n")
    if not shutil.which("g++") or subprocess.run(["gcc"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode:
        pytest.skip("no sanitizer runtime for g++")
    exe = str(tmp_path / "pose_refine_san")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-DPOSE_REFINE_MAIN"] + san + [DRIVER, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header(tmp_path, header):
    names = ("status", "chosen", "R", "t", "err", "R_alt", "t_alt", "err_alt", "err_homography")
    lines = ['printf("%zu", sizeof(amdAprilTagsRefinedPose_t));'] + ['printf(" %%zu", offsetof(amdAprilTagsRefinedPose_t, %s));' % n for n in names]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "apriltag_amd.h"\nint main(void){ %s return 0; }\n' % " ".join(lines))
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    row = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert row == [C.sizeof(capi.RefinedPose)] + [getattr(capi.RefinedPose, n).offset for n in names]
    assert header.lib.pose_refine_sizes(0) == C.sizeof(capi.RefinedPose) == 224
    assert header.lib.pose_refine_sizes(1) == capi.RefinedPose.err_homography.offset
    assert header.lib.pose_refine_sizes(2) == capi.MAX_POSE_ITERATIONS == 200
    assert (capi.POSE_REFINED, capi.POSE_REFINED_NO_ALT, capi.POSE_DEGENERATE) == (pr.REFINED, pr.REFINED_NO_ALT, pr.DEGENERATE) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "apriltag_amd.h")).read()
    for text in ("#define AMDAT_POSE_REFINED 0u", "#define AMDAT_POSE_REFINED_NO_ALT 1u", "#define AMDAT_POSE_DEGENERATE 2u",
                 "#define AMDAT_MAX_POSE_ITERATIONS 200u"):
        assert text in hdr


def test_library_refuses_without_a_device(built):
    """amdAprilTagsSetPoseRefinement / GetRefinedPoses: the null handle, before any HIP call."""
    if not os.path.exists(capi.LIB_PATH):
        build.build_amd()
    L = capi.lib()
    n = C.c_uint32(0)
    rec = capi.RefinedPose()
    assert L.amdAprilTagsSetPoseRefinement(None, 0) == INVALID_ARGUMENT
    assert L.amdAprilTagsSetPoseRefinement(None, 50) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetRefinedPoses(None, 0, C.byref(rec), 1, C.byref(n)) == INVALID_ARGUMENT


def test_node_view_refuses_options_it_would_drop(built):
    """node.py serves pose_refinement alone among the extensions: a second one is an error, not silently ignored."""
    from isaac_ros_apriltag_amd import node
    build.build_node()
    for kw in ({"quad_sigma": 0.8}, {"rectify": True}, {"resize": (640, 480)}, {"bundles": [{"name": "b", "members": [(0, 0.0, 0.0, 0.1)]}]}):
        with pytest.raises(ValueError):
            node.AprilTagNode(pose_refinement=50, **kw)
        with pytest.raises(ValueError):
            node.AprilTagMultiCameraNode(2, pose_refinement=50, **kw)
    with pytest.raises(ValueError):
        node.AprilTagMultiCameraNode(2, pose_refinement=50, max_width=640, max_height=480)
