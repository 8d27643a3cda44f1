"""CPU checks of the camera rigs (amdAprilTagsSetRig): the header csrc/rig_pose.h compiled by g++ against the
Python reference tests/rig_pose_ref.py bit for bit on every case of the GPU test and of this file (also under the host sanitizers in
a program of its own), the ABI, the reference against exact projections and against a numpy minimiser of the same error, the
one-camera identity rig against tests/rigid_bundle_ref.py, the oracle-side preconditions of the GPU cases, and the wrong builds'
forms."""
import ctypes as C
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from isaac_ros_apriltag_amd import capi  # noqa: E402
import bundle_cases as bc  # noqa: E402
import pose_refine_ref as pr  # noqa: E402
import rig_cases as gc  # noqa: E402
import rig_pose_ref as gr  # noqa: E402
import rigid_bundle_cases as rc  # noqa: E402
import rigid_bundle_ref as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "aux_c", "rig_pose_driver.cpp")
_cache = {}


def groups():
    """Every (name, group, bundle) this file and the GPU test solve."""
    if "groups" not in _cache:
        out = []
        for lay in ("cube", "split"):
            for smap in (gc.SLOTS4, gc.SLOTS_ABSENT):
                frames, sl = gc.frames_of([gc.pair_records(s) for s in range(4)], gc.INTR4, gc.SKEW4, smap, gc.PAIR)
                for g in range(4):
                    grp = [dict(frames[i], slot=i) for i in range(4) if sl[i][0] == g and sl[i][1] is not None]
                    out += [("%s:%s:g%d:%s" % (lay, "absent" if smap is gc.SLOTS_ABSENT else "default", g, b["name"]), grp, b) for b in gc.LAYOUTS[lay]]
        frames, sl = gc.frames_of([bc.records72()] * 2, [bc.INTR2] * 2, [0.0, 0.0], ((0, 0), (0, 1)), gc.PAIR72)
        out += [(b["name"], [dict(f, slot=i) for i, f in enumerate(frames)], b) for b in (gc.FULL, gc.OVER)]
        frames, sl = gc.frames_of([gc.dup_records(0), gc.dup_records(1)], gc.DUP_INTR, gc.DUP_SKEW, ((0, 0), (0, 1)), gc.PAIR)
        out.append(("dup", [dict(f, slot=i) for i, f in enumerate(frames)], rc.BUNDLE1))
        for name in gc.TRUTH_RIGS:
            for noise in (0.0, 0.2):
                out.append(("truth:%s:%.1f" % (name, noise), _truth_group(name, noise), dict(gc.CUBE, iterations=200)))
        _cache["groups"] = out
    return _cache["groups"]


def _truth_group(name, noise):
    cams, intr, skews = gc.TRUTH_RIGS[name]
    return gc.exact_group(cams, intr, skews, gc.TRUTH_POSE[0], gc.TRUTH_POSE[1], noise)


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rig_pose") / "librig_pose.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", DRIVER, "-o", so])
    L = C.CDLL(so)
    D = C.POINTER(C.c_double)
    L.rig_pose_probe.argtypes = [C.c_uint32] + [D] * 7 + [C.c_uint32, C.POINTER(capi.RigBundlePose)]
    L.rig_pose_probe.restype = C.c_int
    L.rig_pose_sizes.restype = C.c_uint32
    return L


def _flat(rows):
    v = [float(x) for r in rows for x in np.asarray(r, dtype=np.float64).reshape(-1)]
    return (C.c_double * max(len(v), 1))(*v)


def _header_solve(L, group, bundle):
    """The record of rig_pose.h, fed what the reference reads of the group."""
    obs, nskipped, ndropped, ncams, pix, obj, cams, hom, mem = gr.inputs(group, bundle, gc.FAMS)
    out = gr.zero_record(0, 0, len(obs), nskipped, ndropped, ncams)
    if len(obs) < int(bundle.get("min_tags", 1)) or not obs:
        return out
    o = capi.RigBundlePose()
    cam17 = [list(c[:5]) + list(c[5]) + list(c[6]) for c in cams]
    assert L.rig_pose_probe(len(obs), _flat(pix), _flat(obj), _flat(cam17), _flat([h[0] for h in hom]), _flat([h[1] for h in hom]),
                            _flat([m[0] for m in mem]), _flat([m[1] for m in mem]), int(bundle["iterations"]), C.byref(o)) == 0
    fr, i, _ = obs[int(o.seed)]
    out.update(status=int(o.status), seed_frame=int(fr["slot"]), seed=i, chosen=int(o.chosen), R=np.array(list(o.R)).reshape(3, 3),
               t=np.array(list(o.t)), err=float(o.err), sq_err_sum=float(o.sq_err_sum), R_alt=np.array(list(o.R_alt)).reshape(3, 3),
               t_alt=np.array(list(o.t_alt)), err_alt=float(o.err_alt), sq_err_sum_alt=float(o.sq_err_sum_alt))
    return out


def test_header_equals_the_reference(built, header):
    """csrc/rig_pose.h under g++ against the Python reference on every group of the GPU test and of this file, every double as its 64
    bits."""
    errs, solved = [], 0
    for (name, grp, b) in groups():
        want = gr.solve(grp, b, gc.FAMS)
        solved += want["status"] == gr.SOLVED
        errs += gr.compare(_header_solve(header, grp, b), want, name + ": ")
    print(errs[:10])
    assert not errs and solved >= 12


def test_header_under_asan_ubsan(tmp_path):
    """The same header in a program of its own (the driver's main), built with -fsanitize=address,undefined and run here."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void){return 0;}\n")
    if not shutil.which("g++") or subprocess.run(["gcc"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode:
        pytest.skip("no sanitizer runtime for g++")
    exe = str(tmp_path / "rig_pose_san")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-DRIG_POSE_MAIN"] + san + [DRIVER, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])


def test_struct_layouts_match_the_header(header):
    assert header.rig_pose_sizes(0) == C.sizeof(capi.RigBundlePose) and header.rig_pose_sizes(1) == C.sizeof(capi.RigCamera)
    assert header.rig_pose_sizes(2) == C.sizeof(capi.RigSlot)
    assert header.rig_pose_sizes(3) == capi.MAX_RIG_OBSERVATIONS == gr.SLOTS == header.rig_pose_sizes(5)
    assert header.rig_pose_sizes(4) == capi.MAX_RIG_CAMERAS
    assert set(("amdAprilTagsSetRig", "amdAprilTagsSetRigSlots", "amdAprilTagsGetRigBundlePoses")) <= set(capi.EXPORTS)


def test_library_refuses_without_a_device(built):
    """The entry points exist and refuse a null handle before any device call."""
    if not os.path.exists(capi.LIB_PATH):
        pytest.skip("the HIP library is not built here")
    L = capi.lib()
    assert L.amdAprilTagsSetRig(None, 0, None) == 1 and L.amdAprilTagsSetRigSlots(None, 0, None) == 1
    assert L.amdAprilTagsGetRigBundlePoses(None, None, 0) == 1


# ---- the reference against truth and against a numpy minimiser ---------------------------------------------------------------------------
TRUTH_ROT_DEG, TRUTH_T_M = 16 * 3.55e-14, 16 * 1.0e-15      # 16 x the largest error measured below (see the docstring)
NUMPY_ROT_DEG, NUMPY_T_M = 16 * 2.27e-14, 16 * 1.12e-15


def _minimise(group, bundle):
    """Gauss-Newton with numpy.linalg.lstsq on the residuals (I - F_j)(R P_j + t - o_j), in numpy doubles, from the start of the
    reference's chain 0: the seed's homography pose composed with its member's inverse and moved into the rig frame."""
    _, _, _, _, pix, obj, cams, hom, mem = gr.inputs(group, bundle, gc.FAMS)
    seed = max(range(len(pix)), key=lambda s: (rr.area2(pix[s]), -s))
    R0, t0 = gr.from_camera(cams[seed][5], cams[seed][6], *rr.compose_start(hom[seed][0], hom[seed][1], mem[seed][0], mem[seed][1]))
    P, Fs, os_ = [], [], []
    for tp, to, (fx, fy, cx, cy, skew, Rc, tc) in zip(pix, obj, cams):
        Rc, tc = np.array(Rc).reshape(3, 3), np.array(tc)
        for k in range(4):
            vn = (tp[k][1] - cy) / fy
            un = ((tp[k][0] - cx) - skew * vn) / fx
            d = Rc.T @ np.array([un, vn, 1.0])
            P.append(to[k])
            Fs.append(np.eye(3) - np.outer(d, d) / (d @ d))
            os_.append(-Rc.T @ tc)
    P, Fs, os_ = np.array(P), np.array(Fs), np.array(os_)
    R, t = np.array(R0, dtype=np.float64).reshape(3, 3), np.array(t0, dtype=np.float64)

    def skew_of(w):
        return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])

    def expm(w):
        th = np.linalg.norm(w)
        if th < 1e-300:
            return np.eye(3)
        K = skew_of(w / th)
        return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)

    for _ in range(30):
        X = P @ R.T + t - os_
        res = np.einsum("nij,nj->ni", Fs, X).reshape(-1)
        J = np.zeros((len(P) * 3, 6))
        for j in range(len(P)):
            J[3 * j:3 * j + 3, :3] = Fs[j] @ (-skew_of(R @ P[j]))
            J[3 * j:3 * j + 3, 3:] = Fs[j]
        step = np.linalg.lstsq(J, -res, rcond=None)[0]
        R = expm(step[:3]) @ R
        t = t + step[3:]
    X = P @ R.T + t - os_
    return R, t, float((np.einsum("nij,nj->ni", Fs, X) ** 2).sum())


def test_reference_against_truth_and_numpy(built):
    """Exact projections of the cube (rc.CUBE_MEMBERS) into the two- and the three-camera rig -- distinct float intrinsics per camera,
    a skew on one, non-trivial extrinsics -- and 200 iterations: the reference's pose equals the truth.  Measured here: rotation
    errors up to 3.55e-14 degrees and translation errors up to 1.0e-15 m (the reference's own rounding); asserted: 16 x that
    (5.68e-13 degrees, 1.6e-14 m).  With a deterministic corner noise of 0.2 px the pose is compared with a numpy Gauss-Newton
    minimiser (numpy.linalg.lstsq steps) of the same E from the same start: measured up to 2.27e-14 degrees and 1.12e-15 m apart;
    asserted: 16 x that (3.63e-13 degrees, 1.79e-14 m)."""
    worst = {"truth": [0.0, 0.0], "numpy": [0.0, 0.0]}
    for name in gc.TRUTH_RIGS:
        b = dict(gc.CUBE, iterations=200)
        exact = gr.solve(_truth_group(name, 0.0), b, gc.FAMS)
        assert exact["status"] == gr.SOLVED and exact["nobs"] == 12 * len(gc.TRUTH_RIGS[name][0]) and exact["ncams"] == len(gc.TRUTH_RIGS[name][0])
        dr, dt = rc.pose_errors(exact["R"], exact["t"], *gc.TRUTH_POSE)
        print("truth %s: rotation %.3e deg, translation %.3e m, err %.3e" % (name, dr, dt, exact["err"]))
        worst["truth"] = [max(worst["truth"][0], dr), max(worst["truth"][1], dt)]
        noisy = gr.solve(_truth_group(name, 0.2), b, gc.FAMS)
        Rn, tn, En = _minimise(_truth_group(name, 0.2), b)
        dr, dt = rc.pose_errors(noisy["R"], noisy["t"], Rn, tn)
        print("numpy %s: rotation %.3e deg, translation %.3e m, E %.6e against numpy's %.6e" % (name, dr, dt, noisy["err"], En))
        worst["numpy"] = [max(worst["numpy"][0], dr), max(worst["numpy"][1], dt)]
        assert noisy["err"] > 1e-9 and abs(noisy["err"] - En) <= 1e-9 * En
    print("worst", worst)
    assert worst["truth"][0] <= TRUTH_ROT_DEG and worst["truth"][1] <= TRUTH_T_M
    assert worst["numpy"][0] <= NUMPY_ROT_DEG and worst["numpy"][1] <= NUMPY_T_M


# ---- the identity property -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("cube_a", "one_face"))
def test_one_camera_identity_rig_is_the_rigid_record(built, header, name):
    """A rig of one camera with Rc exactly the identity and tc = 0: the rig record equals rigid_bundle_ref's record of the frame bit
    for bit in R, t, err, sq_err_sum, the alternative fields, chosen and status -- from the reference and from the header."""
    slot = rc.CUBE_FRAMES.index(name)
    for bi, b in enumerate(rc.CUBE_BUNDLES):
        group = [{"slot": 0, "records": rc.cube_records(name), "intrinsics": bc.INTR1[slot], "skew": bc.SKEW1[slot], "camera": (np.eye(3), np.zeros(3))}]
        want = rc.cube_solved(name)[bi]
        for got in (gr.solve(group, b, gc.FAMS, 0, bi), _header_solve(header, group, b)):
            assert got["status"] == want["status"] and got["chosen"] == want["chosen"] and got["nobs"] == want["ntags"]
            assert got["nskipped"] == want["nskipped"] and got["seed"] == want["seed"] and got["seed_frame"] == 0
            for k in rr.FIELDS:
                assert np.array_equal(rr.bits(got[k]), rr.bits(want[k])), (name, b["name"], k)
    assert rc.cube_solved(name)[0]["status"] == rr.SOLVED


# ---- the oracle-side preconditions of the GPU cases -------------------------------------------------------------------------------------------
def test_gpu_preconditions_on_the_oracle_side(built):
    """Which tags each rendered frame holds; nobs, ndropped and ncams per case; that in the split case neither camera alone reaches
    min_tags; that the slot cases have used records in the second 64-record chunk."""
    for slot in range(4):
        recs = gc.pair_records(slot)
        assert sorted(int(r["id"]) for r in recs) == list(gc.SEEN[slot % 2]) and all(int(r["hamming"]) == 0 for r in recs), slot
    cube = gc.pair_solved("cube")
    assert [(g[0]["status"], g[0]["nobs"], g[0]["ncams"], g[0]["ndropped"], g[0]["nskipped"]) for g in cube] == \
        [(0, 16, 2, 0, 0), (0, 16, 2, 0, 0), (1, 0, 0, 0, 0), (1, 0, 0, 0, 0)]
    split = gc.pair_solved("split")
    for g in (0, 1):
        assert (split[g][0]["status"], split[g][0]["nobs"], split[g][0]["ncams"]) == (0, 2, 2)
        assert (split[g][1]["status"], split[g][1]["nobs"], split[g][1]["ncams"]) == (0, 2, 2)
        for slot in (2 * g, 2 * g + 1):   # each camera alone: one tag of the split bundle, below min_tags = 2
            alone = rr.solve(gc.pair_records(slot), gc.SPLIT, gc.FAMS, gc.INTR4[slot], gc.SKEW4[slot])
            assert alone["status"] == rr.TOO_FEW_TAGS and alone["ntags"] == 1
    absent = gc.pair_solved("cube", gc.SLOTS_ABSENT)
    assert [(g[0]["status"], g[0]["nobs"], g[0]["ncams"]) for g in absent] == [(0, 8, 1), (1, 0, 0), (0, 16, 2), (1, 0, 0)]
    assert not absent[1][0]["R"].any() and absent[1][0]["err"] == 0.0
    full, over = gc.solved72("full")[0][0], gc.solved72("over")[0][0]
    assert (full["status"], full["nobs"], full["ndropped"], full["ncams"]) == (0, 64, 0, 2)
    assert (over["status"], over["nobs"], over["ndropped"], over["ncams"]) == (0, 64, 2, 2)
    used, _ = rr.used_slots(bc.records72(), gc.FULL, gc.FAMS)
    assert len(bc.records72()) == 72 and min(i for i, _ in used) < 64 <= max(i for i, _ in used)
    dup = gc.dup_solved()[0][0]
    assert [int(r["id"]) for r in gc.dup_records(0)].count(1) == 2 and [int(r["id"]) for r in gc.dup_records(1)].count(1) == 1
    assert (dup["status"], dup["nobs"], dup["nskipped"], dup["ncams"]) == (0, 5 + 6, 2, 2)   # (id 1: camera 1's observation only)
    obs = gr.gather([dict(records=gc.dup_records(0)), dict(records=gc.dup_records(1))], rc.BUNDLE1, gc.FAMS)[0]
    assert [int(m[1]) for fr, _, m in obs if fr["records"] is gc.dup_records(0)].count(1) == 0
    assert [int(m[1]) for fr, _, m in obs if fr["records"] is gc.dup_records(1)].count(1) == 1


# ---- the wrong builds' forms -------------------------------------------------------------------------------------------------------------------
def test_wrong_build_forms_change_the_record(built):
    """Each mutant's form, stated in Python, changes the reference's record on its case (builds 46 .. 48 of csrc/tools_hooks.h)."""
    want = gc.pair_solved("cube")
    for forms in ({"origin": False}, {"ray_transpose": False}):
        got = gc.pair_solved("cube", **forms)
        assert gr.compare(got[0][0], want[0][0]) and gr.compare(got[1][0], want[1][0]), forms
    assert not gr.compare(gc.pair_solved("cube", slot_cut=63)[0][0], want[0][0])       # (16 observations: the cut at 63 is not reached)
    assert gr.compare(gc.solved72("full", slot_cut=63)[0][0], gc.solved72("full")[0][0])
    assert gc.solved72("full", slot_cut=63)[0][0]["nobs"] == 63
