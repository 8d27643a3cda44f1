"""Raw-frame mode without a GPU (amdAprilTagsSetCornerUndistortion): csrc/undistort.h compiled by a host compiler
against tests/undistort_ref.py bit for bit (and once under AddressSanitizer and UBSan as a program of its own), the properties of the
reference, the point of the feature on the oracle -- the undistorted poses of a raw frame are nearer the truth than the raw records' own
-- and the host side of the plumbing."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from isaac_ros_apriltag_amd import build, capi  # noqa: E402
import bundle_cases as bc  # noqa: E402
import bundle_ref as br  # noqa: E402
import camera_models_ref as cm  # noqa: E402
import pose_refine_cases as pc  # noqa: E402
import rectify_cases as rc  # noqa: E402
import rigid_bundle_ref as rr  # noqa: E402
import undistort_cases as uc  # noqa: E402
import undistort_ref as ur  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DRIVER = os.path.join(HERE, "aux_c", "undistort_driver.cpp")
INVALID_ARGUMENT = 1
SIZES = ((1920, 1080), (320, 48))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _grid(w, h):
    """Pixels of a w x h image, its border and a margin outside it: 23 x 17 positions, none on a round number."""
    us, vs = np.meshgrid(np.linspace(-0.05 * w, 1.05 * w, 23) + 0.137, np.linspace(-0.05 * h, 1.05 * h, 17) - 0.291)
    return us.reshape(-1), vs.reshape(-1)


def _driver_args(camera, us, vs):
    K, D, Kn, kind, R = camera
    Rm = np.eye(3) if R is None else np.asarray(R)
    d8 = list(D) + [0.0] * (8 - len(D))
    args = [str(cm.KINDS[kind])] + [float(v).hex() for v in list(rc.k4(K)) + d8 + list(Rm.reshape(-1)) + list(rc.k4(Kn))]
    for a, b in zip(us, vs):
        args += [float(a).hex(), float(b).hex()]
    return args


def _run_driver(exe, camera, us, vs, **kw):
    out = subprocess.run([exe] + _driver_args(camera, us, vs), capture_output=True, text=True, check=True, **kw).stdout.split("\n")
    rows = [line.split() for line in out if line]
    return (np.array([int(r[0]) for r in rows], dtype=bool), np.array([int(r[1], 16) for r in rows], dtype=np.uint64),
            np.array([int(r[2], 16) for r in rows], dtype=np.uint64))


# ---- 1. the header's lines under a host compiler -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("undistort") / "undistort_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", DRIVER, "-o", exe])
    return exe


def _invalid_cameras():
    return {"folded": uc.FOLDED, "behind": uc.BEHIND, "narrow fisheye": uc.FISHEYE_NARROW}


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", cm.CAMERA_NAMES)
def test_header_equals_the_reference(driver, name, size):
    """undistort of 391 pixels of every camera of camera_models_ref.cameras() at 1920 x 1080 and 320 x 48, bit for bit."""
    w, h = size
    camera = cm.cameras(w, h)[name]
    us, vs = _grid(w, h)
    ok, ub, vb = _run_driver(driver, camera, us, vs)
    uo, vo, want_ok = ur.undistort(us, vs, *camera)
    assert ok.size == us.size and np.array_equal(ok, want_ok)
    assert np.array_equal(ub, _bits(uo)) and np.array_equal(vb, _bits(vo))
    assert want_ok.all()   # (these cameras invert everywhere on and about their image)


@pytest.mark.parametrize("name", ("folded", "behind", "narrow fisheye"))
def test_header_equals_the_reference_where_points_are_invalid(driver, name):
    """The cameras that make INVALID points, on the 640 x 480 grid: the same flags and the same bits, zeros where invalid."""
    camera = _invalid_cameras()[name]
    us, vs = _grid(uc.W, uc.H)
    ok, ub, vb = _run_driver(driver, camera, us, vs)
    uo, vo, want_ok = ur.undistort(us, vs, *camera)
    assert np.array_equal(ok, want_ok) and np.array_equal(ub, _bits(uo)) and np.array_equal(vb, _bits(vo))
    assert not want_ok.all() and not ub[~ok].any() and not vb[~ok].any()
    assert np.isfinite(uo).all() and np.isfinite(vo).all()


def test_header_under_asan_ubsan(tmp_path):
    """The same driver as a program of its own, built with -fsanitize=address,undefined and run here on every camera, the invalid
    ones and non-finite pixels included."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    exe = str(tmp_path / "undistort_san")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra"] + san + [DRIVER, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    cams = dict(cm.cameras(320, 48), **_invalid_cameras())
    for name, camera in cams.items():
        us, vs = _grid(320, 48)
        us = np.concatenate([us, [float("nan"), float("inf"), 1e300]])
        vs = np.concatenate([vs, [0.0, 0.0, -1e300]])
        r = subprocess.run([exe] + _driver_args(camera, us, vs), capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0 and not r.stderr and len(r.stdout.split("\n")) == us.size + 1, (name, r.stderr[-3000:])
        assert r.stdout.split("\n")[-4:-1] == ["0 %016x %016x" % (0, 0)] * 3, name   # the non-finite pixels: invalid, zeros


# ---- 2. properties of the reference ------------------------------------------------------------------------------------------------------------
def _forward(uo, vo, camera):
    """Section 7b's projection of ideal pixels, as camera_models_ref.project states it for a pixel grid, at arbitrary positions."""
    K, D, Kn, kind, R = camera
    K, Kn = np.asarray(K, dtype=np.float64), np.asarray(Kn, dtype=np.float64)
    Ri = (np.eye(3) if R is None else np.asarray(R, dtype=np.float64)).T.reshape(-1)
    xp, yp = (uo - Kn[0, 2]) / Kn[0, 0], (vo - Kn[1, 2]) / Kn[1, 1]
    X, Y, Wd = (Ri[0] * xp + Ri[1] * yp) + Ri[2], (Ri[3] * xp + Ri[4] * yp) + Ri[5], (Ri[6] * xp + Ri[7] * yp) + Ri[8]
    xd, yd = ur.distort(X / Wd, Y / Wd, D, kind)
    return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]


def _round_trip_cases():
    out = [("%s %dx%d" % (n, w, h), (n, (w, h))) for (w, h) in SIZES for n in cm.CAMERA_NAMES]
    return out + [("%s 640x480 short lens" % n, (n, None)) for n in uc.CAMERA_NAMES]


@pytest.mark.parametrize("label,case", _round_trip_cases())
def test_projection_of_the_undistorted_pixel_is_the_pixel(label, case):
    """project(undistort(q)) = q within the gate, 2^-20 px, for every converged pixel: section 7b's projection, written out here for
    arbitrary positions, applied to the reference's result."""
    name, size = case
    camera, (w, h) = (uc.CAMERAS[name], (uc.W, uc.H)) if size is None else (cm.cameras(*size)[name], size)
    us, vs = _grid(w, h)
    uo, vo, ok = ur.undistort(us, vs, *camera)
    assert ok.all()
    fu, fv = _forward(uo, vo, camera)
    err = float(max(np.abs(fu - us).max(), np.abs(fv - vs).max()))
    print("%s: round trip %.3g px" % (label, err))
    assert err <= ur.GATE_PX


def test_no_distortion_is_the_identity():
    """D = 0, R = I, Knew = K: |p_u - p| <= 1e-9 px."""
    for w, h in SIZES:
        K = rc.camera(w, h)
        us, vs = _grid(w, h)
        for kind, D in (("plumb_bob", [0.0] * 5), ("rational_polynomial", [0.0] * 8)):
            uo, vo, ok = ur.undistort(us, vs, K, D, K, kind, None)
            assert ok.all() and float(max(np.abs(uo - us).max(), np.abs(vo - vs).max())) <= 1e-9


def test_plumb_bob_is_rational_with_a_unit_denominator():
    for w, h in SIZES:
        K, D, Kn, _, _ = cm.cameras(w, h)["plumb_bob"]
        us, vs = _grid(w, h)
        a = ur.undistort(us, vs, K, D, Kn, "plumb_bob", None)
        b = ur.undistort(us, vs, K, list(D) + [0.0] * 3, Kn, "rational_polynomial", None)
        assert all(np.array_equal(_bits(x.astype(np.float64)), _bits(y.astype(np.float64))) for x, y in zip(a, b))


def test_each_invalid_cause():
    """A folded polynomial (k = -0.35, 0.15, -0.03: r * radial(r) turns back at r = 1.51, where it is 0.944, so a distorted radius of 1.0
    has no preimage), a ray with W <= 0 under a large R, a fisheye radius beyond 90 degrees."""
    K = uc.K_RAW
    u = np.array([K[0, 2] + 1.0 * K[0, 0]])
    v = np.array([K[1, 2]])
    uo, vo, ok = ur.undistort(u, v, *uc.FOLDED)
    assert not ok[0] and uo[0] == 0.0 and vo[0] == 0.0
    # (at xd = 0.8 the same polynomial still has the preimage x = 1.08: whatever the iteration does there, the gate decides, and a point
    # it lets through is a true preimage)
    uo, vo, ok = ur.undistort(np.array([K[0, 2] + 0.8 * K[0, 0]]), v, *uc.FOLDED)
    print("folded polynomial at xd = 0.8: ok %s, x = %r" % (bool(ok[0]), (uo[0] - uc.KNEW[0, 2]) / uc.KNEW[0, 0]))
    assert not ok[0] or abs(_forward(uo, vo, uc.FOLDED)[0][0] - u[0] + 0.2 * K[0, 0]) <= ur.GATE_PX
    assert ur.undistort(np.array([K[0, 2] + 0.1 * K[0, 0]]), v, *uc.FOLDED)[2][0]      # near the axis the same camera inverts
    us, vs = _grid(uc.W, uc.H)
    behind = ur.undistort(us, vs, *uc.BEHIND)[2]
    assert not behind[us > 0.5 * uc.W].any() and behind.any()   # (W = cos(100 deg) - sin(100 deg) x: only the far left still looks forward)
    Kf = uc.FISHEYE_NARROW[0]
    thd_max = math.pi / 2 * (1 + sum(k * (math.pi / 2) ** (2 * (i + 1)) for i, k in enumerate(uc.D_FISHEYE)))   # theta_d at 90 degrees
    beyond = np.array([Kf[0, 2] + Kf[0, 0] * (thd_max + 0.05)])
    inside = np.array([Kf[0, 2] + Kf[0, 0] * (thd_max - 0.2)])
    assert not ur.undistort(beyond, np.array([Kf[1, 2]]), *uc.FISHEYE_NARROW)[2][0]
    assert ur.undistort(inside, np.array([Kf[1, 2]]), *uc.FISHEYE_NARROW)[2][0]
    deg87 = np.array([Kf[0, 2] + Kf[0, 0] * math.radians(87.0) * (1 + sum(k * math.radians(87.0) ** (2 * (i + 1)) for i, k in enumerate(uc.D_FISHEYE)))])
    uo, vo, ok = ur.undistort(deg87, np.array([Kf[1, 2]]), *uc.FISHEYE_NARROW)
    assert ok[0] and abs((uo[0] - uc.KNEW[0, 2]) / uc.KNEW[0, 0] - math.tan(math.radians(87.0))) < 1e-6   # 87 degrees off axis converges


def test_an_invalid_record_gives_finite_values_in_every_consumer(built):
    """The nine-tag frame's records with tag 4's corners moved to where the folded camera has no preimage: the twin is INVALID with zero
    fields, the planar and the rigid bundle skip it and count it, its refined record is DEGENERATE with zero fields, its covariance all
    zero -- and nothing anywhere is NaN or infinite."""
    recs = [dict(r) for r in uc.raw_records("nine", "plumb_bob")]
    K = uc.K_RAW
    bad = [i for i, r in enumerate(recs) if int(r["id"]) == 4][0]
    recs[bad]["p"] = np.asarray(recs[bad]["p"]) + np.array([1.1 * K[0, 0], 0.0])
    tw = ur.records(recs, uc.FOLDED, uc.INTR, bc.SIZE1)
    assert [t["status"] for t in tw] == [ur.INVALID if i == bad else ur.OK for i in range(9)]
    z = tw[bad]
    assert z["hamming_dev"] == ur.INT32_MAX and not any(np.asarray(z[k]).any() for k in ("H", "center", "p", "R", "t"))
    feed = ur.for_consumers(tw)
    planar = br.solve(feed, uc.BUNDLE9, list(bc.FAM), uc.INTR)
    rigid = rr.solve(feed, uc.RIGID9, list(bc.FAM), uc.INTR)
    assert (planar["status"], planar["ntags"], planar["nskipped"]) == (br.SOLVED, 8, 1)
    assert (rigid["status"], rigid["ntags"], rigid["nskipped"]) == (rr.SOLVED, 8, 1)
    refined = ur.refined(tw, uc.INTR, 0.0, bc.SIZE1, pc.ITERATIONS)
    covs = ur.covariances(tw, uc.INTR, 0.0, bc.SIZE1, refined, 0.3)
    assert refined[bad]["status"] == ur.POSE_DEGENERATE and covs[bad]["valid"] == 0
    for rec in tw + [planar, rigid] + refined + covs:
        for k, val in rec.items():
            if isinstance(val, (float, np.ndarray)):
                assert np.isfinite(np.asarray(val, dtype=np.float64)).all(), k
    assert not any(np.asarray(refined[bad][k]).any() for k in ("R", "t", "err", "R_alt", "t_alt", "err_alt", "err_homography"))
    assert not any(np.asarray(covs[bad][k]).any() for k in ("cov", "cov_alt", "sq_err_sum", "sq_err_sum_alt"))


# ---- 3. end to end on the oracle: the point of the feature ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ("plumb_bob", "rational", "equidistant") + tuple(uc.SAME_FOCAL))
@pytest.mark.parametrize("name", ("oblique", "cube_a"))
def test_undistorted_poses_are_nearer_the_truth_than_the_raw_ones(built, name, cam):
    """The ideal frame seen through each kind of camera: every id of the ideal frame is found on the raw frame, and the median
    translation error of the undistorted poses against the analytic truth is smaller than that of the raw records' own poses.  (Printed
    beside them: the oracle on the rectified raw frame, and on the ideal frame itself.)  The cameras: the short lens of each kind, whose
    raw poses are wrong mostly by its focal length, and the "=f" cameras with the ideal camera's own focal length and stronger
    coefficients, whose raw poses are wrong by the distortion alone."""
    ideal, raw, twins = uc.ideal_records(name), uc.raw_records(name, cam), uc.twins(name, cam)
    assert sorted(int(r["id"]) for r in ideal) == sorted(uc.truth(name)) == sorted(int(r["id"]) for r in raw)
    assert all(t["status"] == ur.OK for t in twins)
    med = lambda recs: float(np.median(list(uc.translation_errors(recs, name).values())))
    e_raw, e_und, e_rect, e_ideal = med(raw), med(twins), med(uc.rectified_records(name, cam)), med(ideal)
    print("%s %s: median |t - t_true| in mm: raw %.2f, undistorted %.3f, rectified %.3f, ideal frame %.3f" %
          (name, cam, 1e3 * e_raw, 1e3 * e_und, 1e3 * e_rect, 1e3 * e_ideal))
    assert e_und < e_raw


def test_gpu_preconditions_on_the_reference_side(built):
    """What tests/test_corner_undistortion_gpu.py relies on: nine, none and one record on the three raw frames under each slot's camera;
    the wrong builds' forms give other twins exactly where that test expects it; hooks 28 .. 30 are registered."""
    for slot, (name, n) in enumerate((("nine", 9), ("none", 0), ("one", 1))):
        assert len(uc.raw_records(name, uc.KINDS3[slot])) == n
    # 28: R as the identity -- another twin under a camera with R, the same one without
    assert ur.compare(uc.twins("nine", "plumb_bob+R", rotation=False)[0], uc.twins("nine", "plumb_bob+R")[0])
    assert not ur.compare(uc.twins("nine", "rational", rotation=False)[0], uc.twins("nine", "rational")[0])
    # 30: slot 2 under slot 0's camera
    assert ur.compare(uc.twins("one", uc.KINDS3[2], camera=uc.CAMERAS[uc.KINDS3[0]])[0], uc.twins("one", uc.KINDS3[2])[0])
    # 29: the bundle of the raw records is not the bundle of the twins
    raw, tw = uc.raw_records("nine", uc.KINDS3[0]), ur.for_consumers(uc.twins("nine", uc.KINDS3[0]))
    assert br.compare(br.solve(raw, uc.BUNDLE9, list(bc.FAM), uc.INTR), br.solve(tw, uc.BUNDLE9, list(bc.FAM), uc.INTR))
    hooks = open(os.path.join(ROOT, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    for n in (28, 29, 30):
        assert n in build.MUTANTS and "AMDAT_MUTATE == %d" % n in hooks


# ---- 4. plumbing ---------------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header(tmp_path):
    names = ("status", "reserved", "H", "c", "p", "R", "t")
    t = "amdAprilTagsUndistortedDetection_t"
    lines = ['printf("%%zu", sizeof(%s));' % t] + ['printf(" %%zu", offsetof(%s, %s));' % (t, n) for n in names] + \
            ['printf(" %d %u %u", AMDAT_UNDISTORT_ITERATIONS, AMDAT_UNDISTORT_OK, AMDAT_UNDISTORT_INVALID);']
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "apriltag_amd.h"\n#include "apriltag_amd_debug.h"\nint main(void){ %s return 0; }\n' % " ".join(lines))
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    row = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert row[:8] == [C.sizeof(capi.UndistortedDetection)] + [getattr(capi.UndistortedDetection, n).offset for n in names]
    assert row[:8] == [capi.UNDISTORTED_DTYPE.itemsize] + [capi.UNDISTORTED_DTYPE.fields[n][1] for n in names]
    assert row[8:] == [capi.UNDISTORT_ITERATIONS, capi.UNDISTORT_OK, capi.UNDISTORT_INVALID] == [ur.ITERATIONS, ur.OK, ur.INVALID]
    for name in ("amdAprilTagsSetCornerUndistortion", "amdAprilTagsGetUndistortedDetections", "amdAprilTagsDebugUndistort"):
        assert name in capi.EXPORTS


def test_library_refuses_without_a_device(built):
    """The three calls on the null handle, before any HIP call."""
    if not os.path.exists(capi.LIB_PATH):
        build.build_amd()
    L = capi.lib()
    n = C.c_uint32(0)
    rec = capi.UndistortedDetection()
    cam = capi.camera_models_ex([uc.CAMERAS["rational+R"]])
    assert L.amdAprilTagsSetCornerUndistortion(None, 1, cam) == INVALID_ARGUMENT
    assert L.amdAprilTagsSetCornerUndistortion(None, 0, None) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetUndistortedDetections(None, 0, C.byref(rec), 1, C.byref(n)) == INVALID_ARGUMENT
    assert L.amdAprilTagsDebugUndistort(None, 0, None, cam, None, None) == INVALID_ARGUMENT
