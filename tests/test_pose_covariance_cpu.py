"""CPU checks of the pose covariance (amdAprilTagsSetPoseCovariance): the header csrc/pose_covariance.h compiled
by g++ against the Python reference tests/pose_cov_ref.py bit for bit (also under the host sanitizers in a program of its own);
independent checks of the reference -- symmetry, the Jacobian against central differences of the projection, the inverse against
numpy's --; the refusals; the reference-side preconditions of the GPU test; and the ABI."""
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
import pose_cov_ref as pv  # noqa: E402
import pose_refine_cases as pc  # noqa: E402
import pose_refine_ref as pr  # noqa: E402
import rigid_bundle_cases as rc  # noqa: E402
import rigid_bundle_ref as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "aux_c", "pose_cov_driver.cpp")
INVALID_ARGUMENT = 1
INTR = (600.0, 600.0, 320.0, 240.0)
SIZE = float(np.float32(0.1))
SIGMA = 0.3
_cache = {}


def _tag_cases():
    """(label, corners, skew, refined record): 40 seeded poses at tilts 0 .. 80 degrees with 0.3 px of corner noise, under skew 0 and
    0.75 in turn; tilt exactly 0 and a tag at 20 m (exact corners), each under both skews."""
    if "tags" not in _cache:
        rng = np.random.default_rng(71)
        poses = []
        for i in range(40):
            R, t = pc.random_pose(rng, 0.0, 80.0)
            poses.append(("seeded %d" % i, R, t, 0.75 if i % 2 else 0.0, rng.normal(0.0, 0.3, (4, 2))))
        for skew in (0.0, 0.75):
            poses.append(("tilt 0, skew %g" % skew, pc.rodrigues((0.0, 0.0, 1.0), 0.3), np.array([0.05, -0.03, 1.0]), skew, 0.0))
            poses.append(("20 m, skew %g" % skew, pc.rodrigues((math.cos(0.4), math.sin(0.4), 0.0), math.radians(30.0)),
                          np.array([0.5, -0.3, 20.0]), skew, 0.0))
            poses.append(("tilt 0 at 20 m, skew %g" % skew, np.eye(3), np.array([0.5, -0.3, 20.0]), skew, 0.0))
        out = []
        for label, R, t, skew, noise in poses:
            p = pc.project(R, t, INTR, skew, SIZE) + noise
            Rh, th = pc.homography_pose(p, INTR, skew, SIZE)
            out.append((label, p, skew, pr.refine(p, INTR, skew, SIZE, Rh, th, pc.ITERATIONS)))
        _cache["tags"] = out
    return _cache["tags"]


def _bundle_cases():
    """(label, pix, obj, intrinsics, skew, solved record): the cube corner, the coplanar face with its alternative, the lone tag, and
    the bundle with too few tags -- rigid_bundle_cases' three frames under their slots' cameras (slot 1 has a skew)."""
    if "bundles" not in _cache:
        out = []
        for slot, name in enumerate(rc.CUBE_FRAMES):
            for b, bundle in enumerate(rc.CUBE_BUNDLES):
                _, _, pix, obj, _, _ = rr.inputs(rc.cube_records(name), bundle, rc.FAMS, bc.INTR1[slot], bc.SKEW1[slot])
                out.append(("%s / %s" % (name, bundle["name"]), pix, obj, bc.INTR1[slot], bc.SKEW1[slot], rc.cube_solved(name)[b]))
        _cache["bundles"] = out
    return _cache["bundles"]


def _full(N):
    return np.array([[N[pv.ix(max(r, s), min(r, s))] for s in range(6)] for r in range(6)])


# ---- the header ----------------------------------------------------------------------------------------------------------------------------
def _refined_struct(o):
    s = capi.RefinedPose()
    s.status, s.chosen = int(o["status"]), int(o["chosen"])
    for k in ("R", "t", "R_alt", "t_alt"):
        v = np.asarray(o[k], dtype=np.float64).reshape(-1)
        setattr(s, k, (C.c_double * len(v))(*v))
    s.err, s.err_alt, s.err_homography = float(o["err"]), float(o["err_alt"]), float(o["err_homography"])
    return s


def _bundle_struct(o):
    s = capi.BundlePoseEx()
    for k in ("bundle", "status", "ntags", "nskipped", "seed", "chosen"):
        setattr(s, k, int(o[k]))
    for k in ("R", "t", "R_alt", "t_alt"):
        v = np.asarray(o[k], dtype=np.float64).reshape(-1)
        setattr(s, k, (C.c_double * len(v))(*v))
    for k in ("err", "sq_err_sum", "err_alt", "sq_err_sum_alt"):
        setattr(s, k, float(o[k]))
    return s


def _rec(c):
    return {"cov": np.array(list(c.cov)).reshape(6, 6), "cov_alt": np.array(list(c.cov_alt)).reshape(6, 6), "sq_err_sum": float(c.sq_err_sum),
            "sq_err_sum_alt": float(c.sq_err_sum_alt), "valid": int(c.valid), "reserved": int(c.reserved)}


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pose_cov") / "libpose_cov.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", DRIVER, "-o", so])
    L = C.CDLL(so)
    L.pose_cov_tag_probe.argtypes = [C.POINTER(C.c_double)] + [C.c_double] * 6 + [C.POINTER(capi.RefinedPose), C.c_double, C.POINTER(capi.PoseCovariance)]
    L.pose_cov_tag_probe.restype = None
    L.pose_cov_bundle_probe.argtypes = [C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double)] + [C.c_double] * 5 + \
        [C.POINTER(capi.BundlePoseEx), C.c_double, C.POINTER(capi.PoseCovariance)]
    L.pose_cov_bundle_probe.restype = None
    L.pose_cov_sizes.restype = C.c_uint32

    class Probe:
        lib = L

        @staticmethod
        def tag(p, intr, skew, size, refined, sigma):
            o = capi.PoseCovariance()
            p8 = (C.c_double * 8)(*[float(v) for pt in p for v in pt])
            L.pose_cov_tag_probe(p8, *[pr.f32(v) for v in intr], pr.f32(skew), pr.f32(size), C.byref(_refined_struct(refined)), float(sigma), C.byref(o))
            return _rec(o)

        @staticmethod
        def bundle(pix, obj, intr, skew, solved, sigma):
            o = capi.PoseCovariance()
            fp = [float(v) for slot in pix for q in slot for v in q]
            fo = [float(v) for slot in obj for P in slot for v in P]
            L.pose_cov_bundle_probe(len(pix), (C.c_double * max(len(fp), 1))(*fp), (C.c_double * max(len(fo), 1))(*fo), *[pr.f32(v) for v in intr],
                                    pr.f32(skew), C.byref(_bundle_struct(solved)), float(sigma), C.byref(o))
            return _rec(o)
    return Probe


def test_header_equals_the_reference_on_tags(built, header):
    """csrc/pose_covariance.h under g++ against the Python reference, every field bit for bit, on the tag cases; every case has both
    halves (the two minima), and a second sigma scales them."""
    errs = []
    for label, p, skew, refined in _tag_cases():
        for sigma in (SIGMA, 1.25):
            got, want = header.tag(p, INTR, skew, SIZE, refined, sigma), pv.tag_record(p, INTR, skew, SIZE, refined, sigma)
            errs += pv.compare(got, want, "%s, sigma %g: " % (label, sigma))
            assert got["reserved"] == 0
        assert refined["status"] == pr.REFINED and want["valid"] == 3, label
    # a record without an alternative: the second half is zeros with its bit clear
    label, p, skew, refined = _tag_cases()[0]
    lone = dict(refined, status=pr.REFINED_NO_ALT)
    got, want = header.tag(p, INTR, skew, SIZE, lone, SIGMA), pv.tag_record(p, INTR, skew, SIZE, lone, SIGMA)
    errs += pv.compare(got, want, "no alternative: ")
    assert want["valid"] == 1 and not want["cov_alt"].any() and want["sq_err_sum_alt"] == 0.0
    print(errs[:10])
    assert not errs


def test_header_equals_the_reference_on_bundles(built, header):
    """The same through the host tree sum RgSumTree on rigid_bundle_cases' point sets: the cube corner (non-coplanar), one face
    (coplanar, with an alternative), the lone tag, and the zeroed record of a bundle with too few tags."""
    errs, seen = [], set()
    for label, pix, obj, intr, skew, solved in _bundle_cases():
        got, want = header.bundle(pix, obj, intr, skew, solved, SIGMA), pv.bundle_record(pix, obj, intr, skew, solved, SIGMA)
        errs += pv.compare(got, want, label + ": ")
        seen.add((int(solved["status"]), want["valid"], len(pix) > 1))
        if solved["status"] == rr.TOO_FEW_TAGS:
            assert want["valid"] == 0 and not want["cov"].any() and not want["cov_alt"].any()
        else:
            assert want["valid"] & 1 and (want["valid"] == 3) == bool(np.asarray(solved["R_alt"]).any()), label
            assert want["sq_err_sum"] == 0.0 and want["sq_err_sum_alt"] == 0.0
    print(sorted(seen), errs[:10])
    assert not errs
    # several tags, a one-tag bundle (both chains of a solved bundle ran: it has an alternative), a bundle with too few tags
    assert (rr.SOLVED, 3, True) in seen and (rr.SOLVED, 3, False) in seen and (rr.TOO_FEW_TAGS, 0, False) in seen


def test_header_under_asan_ubsan(tmp_path):
    """The same header in a program of its own (the driver's main), built with -fsanitize=address,undefined and run here."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void){return 0;}\n")
    if not shutil.which("g++") or subprocess.run(["gcc"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode:
        pytest.skip("no sanitizer runtime for g++")
    exe = str(tmp_path / "pose_cov_san")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-DPOSE_COV_MAIN"] + san + [DRIVER, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])


# ---- independent checks of the reference ---------------------------------------------------------------------------------------------------
def _project(P, R, t, cam):
    fx, fy, cx, cy, skew = cam
    X = np.asarray(R).reshape(3, 3) @ np.asarray(P) + np.asarray(t)
    return np.array([(fx * X[0] + skew * X[1]) / X[2] + cx, fy * X[1] / X[2] + cy])


def _all_reference_cases():
    """(label, points, pixels, camera, R, t, sum) of every pose the cases above evaluate at."""
    out = []
    for label, p, skew, refined in _tag_cases():
        cam = INTR + (pr.f32(skew),)
        for k in ("", "_alt"):
            out.append((label + k, pv.tag_points(SIZE), p, cam, refined["R" + k], refined["t" + k], pr.sum4))
    for label, pix, obj, intr, skew, solved in _bundle_cases():
        if solved["status"] == rr.TOO_FEW_TAGS:
            continue
        cam = tuple(pr.f32(v) for v in intr) + (pr.f32(skew),)
        pts = [tuple(P) for slot in obj for P in slot]
        px = [tuple(q) for slot in pix for q in slot]
        for k in ("", "_alt"):
            if np.asarray(solved["R" + k]).any():
                out.append((label + k, pts, px, cam, solved["R" + k], solved["t" + k], pv.tree_sum(len(pix))))
    return out


def test_reference_covariance_is_symmetric_with_a_positive_diagonal(built):
    for label, p, skew, refined in _tag_cases():
        c = pv.tag_record(p, INTR, skew, SIZE, refined, SIGMA)
        for k in ("cov", "cov_alt"):
            assert np.array_equal(c[k], c[k].T) and (np.diag(c[k]) > 0.0).all(), (label, k)
    for label, pix, obj, intr, skew, solved in _bundle_cases():
        c = pv.bundle_record(pix, obj, intr, skew, solved, SIGMA)
        for bit, k in ((1, "cov"), (2, "cov_alt")):
            assert np.array_equal(c[k], c[k].T), (label, k)
            assert (np.diag(c[k]) > 0.0).all() if c["valid"] & bit else not c[k].any(), (label, k)


def test_reference_jacobian_against_central_differences(built):
    """J against central differences of the projection under t' = t + dt, R' = Rodrigues(dtheta) R with the step 2^-17: truncation
    (h^2 times a third derivative of order the row) and rounding (2^-53 / h) each come to about 1e-9 of a row's largest entry; 1e-6 of
    it is allowed, which a wrong sign, index or transposition -- an error of order 1 -- cannot meet."""
    h = 2.0 ** -17
    worst = 0.0
    for label, pts, _, cam, R, t, _ in _all_reference_cases():
        R9 = [float(v) for v in np.asarray(R).reshape(-1)]
        t3 = [float(v) for v in np.asarray(t).reshape(-1)]
        for P in pts[:8]:
            Ju, Jv, u, v = pv.jacobian_rows(P, R9, t3, cam)
            assert np.abs(np.array([u, v]) - _project(P, R9, t3, cam)).max() < 1e-9
            num = np.zeros((2, 6))
            for k in range(6):
                def at(sign):
                    if k < 3:
                        dt = np.zeros(3)
                        dt[k] = sign * h
                        return _project(P, R9, np.asarray(t3) + dt, cam)
                    axis = np.zeros(3)
                    axis[k - 3] = 1.0
                    return _project(P, pc.rodrigues(axis, sign * h) @ np.asarray(R9).reshape(3, 3), t3, cam)
                num[:, k] = (at(1.0) - at(-1.0)) / (2.0 * h)
            for row, J in zip(num, (Ju, Jv)):
                rel = np.abs(row - np.array(J)).max() / np.abs(np.array(J)).max()
                worst = max(worst, rel)
                assert rel < 1e-6, (label, rel)
    print("Jacobian against central differences: worst %.3g of a row's largest entry" % worst)


def test_reference_inverse_against_numpy(built):
    """cov against sigma^2 * numpy.linalg.inv(N) within 64 * cond(N) * 2^-53 * |cov|, the backward-error bound of a 6 x 6 Cholesky,
    cond(N) computed per case."""
    worst_cond, worst_ratio = 0.0, 0.0
    for label, pts, px, cam, R, t, sum_ in _all_reference_cases():
        N, _ = pv.normal(pts, px, [float(v) for v in np.asarray(R).reshape(-1)], [float(v) for v in np.asarray(t).reshape(-1)], cam, sum_)
        ok, cov = pv.invert(N, SIGMA * SIGMA)
        assert ok, label
        Nf = _full(N)
        cond = float(np.linalg.cond(Nf))
        bound = 64.0 * cond * 2.0 ** -53 * float(np.linalg.norm(cov, 2))
        diff = float(np.abs(cov - SIGMA * SIGMA * np.linalg.inv(Nf)).max())
        worst_cond, worst_ratio = max(worst_cond, cond), max(worst_ratio, diff / bound)
        assert diff <= bound, (label, cond, diff, bound)
    print("inverse against numpy: largest cond(N) %.3g, largest share of the bound %.3g" % (worst_cond, worst_ratio))
    assert worst_cond < 1e8


def test_growth_with_distance_from_the_reference(built):
    """The geometry behind the feature: a 0.1 m tag, f = 600 px, 0.3 px of corner noise, the standard deviation of the rotation about
    an in-plane axis.  Tilted by 45 degrees the rotation moves the corners by f s sin(tilt) / z per radian, so the figure grows
    linearly with z; fronto-parallel only the foreshortening f s^2 / z^2 shows it, so it grows with z^2 -- both up to terms of order
    (s / z)^2, 1 % at 0.5 m; 5 % is allowed.  The figures are printed: DESIGN.md section 7g quotes them."""
    got = {}
    for tilt in (45.0, 0.0):
        for z in (0.5, 2.0, 5.0):
            R = pc.rodrigues((1.0, 0.0, 0.0), math.radians(tilt))
            t = np.array([0.0, 0.0, z])
            p = pc.project(R, t, INTR, 0.0, SIZE)
            c = pv.record(pv.tag_points(SIZE), p, INTR + (0.0,), (R, t), None, 0.3, pr.sum4)
            assert c["valid"] == 1
            got[(tilt, z)] = math.degrees(math.sqrt(c["cov"][3, 3]))
            print("tilt %2.0f, z %.1f m: %.3g degrees" % (tilt, z, got[(tilt, z)]))
    for tilt, power in ((45.0, 1.0), (0.0, 2.0)):
        for z0, z1 in ((0.5, 2.0), (2.0, 5.0)):
            assert abs(got[(tilt, z1)] / got[(tilt, z0)] / (z1 / z0) ** power - 1.0) < 0.05, (tilt, z0, z1)
    assert all(got[(0.0, z)] > 4.0 * got[(45.0, z)] for z in (0.5, 2.0, 5.0))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(built, header):
    """Four identical pixels, all object points on one viewing ray, and a NaN in the pose clear the valid bit and give zeros -- in the
    reference and in the header alike."""
    label, p, skew, refined = _tag_cases()[0]
    lone = dict(refined, status=pr.REFINED_NO_ALT)
    # four identical pixels: their homography maps every c_k to one pixel, its pose is not finite, the refinement is degenerate and
    # reports that pose -- and the covariance at it is refused
    from oracle import pyoracle as po
    same = np.full((4, 2), 100.0)
    Rh, th = po.pose_from_homography(np.array([0.0, 0.0, 100.0, 0.0, 0.0, 100.0, 0.0, 0.0, 1.0]), INTR[0], INTR[1], INTR[2], INTR[3], SIZE, skew=0.0)
    with np.errstate(all="ignore"):
        deg = pr.refine(same, INTR, 0.0, SIZE, Rh, th, pc.ITERATIONS)
    assert deg["status"] == pr.DEGENERATE
    cases = [("equal pixels", same, 0.0, deg)]
    nan_t = np.array(lone["t"])
    nan_t[1] = float("nan")
    cases.append(("NaN in t", p, skew, dict(lone, t=nan_t)))
    nan_R = np.array(lone["R"])
    nan_R[2, 0] = float("nan")
    cases.append(("NaN in R", p, skew, dict(lone, R=nan_R)))
    for name, pix, sk, o in cases:
        got, want = header.tag(pix, INTR, sk, SIZE, o, SIGMA), pv.tag_record(pix, INTR, sk, SIZE, o, SIGMA)
        assert want["valid"] == 0 and not want["cov"].any() and not want["cov_alt"].any(), name
        assert not pv.compare(got, want), name
    # all object points on one viewing ray (a bundle "member" whose corners lie along the ray through the principal point)
    ray_obj = [[(0.0, 0.0, 0.1 * k) for k in range(4)]]
    ray_pix = [[(320.0, 240.0)] * 4]
    solved = {"bundle": 0, "status": rr.SOLVED, "ntags": 1, "nskipped": 0, "seed": 0, "chosen": 0, "R": np.eye(3), "t": np.array([0.0, 0.0, 1.0]),
              "err": 0.0, "sq_err_sum": 0.0, "R_alt": np.zeros((3, 3)), "t_alt": np.zeros(3), "err_alt": 0.0, "sq_err_sum_alt": 0.0}
    got, want = header.bundle(ray_pix, ray_obj, INTR, 0.0, solved, SIGMA), pv.bundle_record(ray_pix, ray_obj, INTR, 0.0, solved, SIGMA)
    assert want["valid"] == 0 and not want["cov"].any() and not pv.compare(got, want)


# ---- what the GPU test relies on -----------------------------------------------------------------------------------------------------------
def test_gpu_preconditions_on_the_reference_side(built):
    """The wrong builds' forms of the definition give other records exactly where the GPU test expects it: without the skew term in
    J_u only under a skew; with centred object points for every solved bundle whose points do not average to the origin; hooks 25 .. 27
    are registered."""
    for label, p, skew, refined in _tag_cases():
        a, b = pv.tag_record(p, INTR, skew, SIZE, refined, SIGMA), pv.tag_record(p, INTR, skew, SIZE, refined, SIGMA, skew_in_ju=False)
        assert bool(pv.compare(a, b)) == (skew != 0.0), label
        assert pv.compare({**a, "cov_alt": a["cov"]}, a)   # the two halves differ: "cov_alt equals cov" is another record
    for label, pix, obj, intr, skew, solved in _bundle_cases():
        if solved["status"] != rr.TOO_FEW_TAGS:
            differ = bool(pv.compare(pv.bundle_record(pix, obj, intr, skew, solved, SIGMA, centred=True), pv.bundle_record(pix, obj, intr, skew, solved, SIGMA)))
            assert differ == (len(pix) > 1), label   # (the lone tag's corners average to the origin as they stand)
    hooks = open(os.path.join(ROOT, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    for n in (25, 26, 27):
        assert n in build.MUTANTS and "AMDAT_MUTATE == %d" % n in hooks


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header(tmp_path, header):
    names = ("cov", "cov_alt", "sq_err_sum", "sq_err_sum_alt", "valid", "reserved")
    lines = ['printf("%zu", sizeof(amdAprilTagsPoseCovariance_t));'] + ['printf(" %%zu", offsetof(amdAprilTagsPoseCovariance_t, %s));' % n for n in names]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "apriltag_amd.h"\nint main(void){ %s return 0; }\n' % " ".join(lines))
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    row = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert row == [C.sizeof(capi.PoseCovariance)] + [getattr(capi.PoseCovariance, n).offset for n in names]
    assert row == [capi.POSE_COV_DTYPE.itemsize] + [capi.POSE_COV_DTYPE.fields[n][1] for n in names]
    assert header.lib.pose_cov_sizes(0) == C.sizeof(capi.PoseCovariance) == 600
    assert header.lib.pose_cov_sizes(1) == capi.PoseCovariance.valid.offset
    for name in ("amdAprilTagsSetPoseCovariance", "amdAprilTagsGetRefinedPoseCovariances", "amdAprilTagsGetBundlePoseCovariancesEx"):
        assert name in capi.EXPORTS


def test_library_refuses_without_a_device(built):
    """amdAprilTagsSetPoseCovariance and both getters: the null handle, before any HIP call."""
    if not os.path.exists(capi.LIB_PATH):
        build.build_amd()
    L = capi.lib()
    n = C.c_uint32(0)
    rec = capi.PoseCovariance()
    for sigma in (0.0, 0.3, float("nan"), float("inf"), -1.0):
        assert L.amdAprilTagsSetPoseCovariance(None, sigma) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetRefinedPoseCovariances(None, 0, C.byref(rec), 1, C.byref(n)) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetBundlePoseCovariancesEx(None, C.byref(rec), 0) == INVALID_ARGUMENT
