"""CPU checks of the rigid 3-D tag bundles (amdAprilTagsSetBundlesEx): the headers csrc/rigid_pose.h and
csrc/rigid_layout.h compiled by g++ against the Python reference tests/rigid_bundle_ref.py bit for bit on every scene of the GPU test
(also under the host sanitizers in a program of its own), the layout's refusals, the ABI, the reference's rotation step against
numpy's SVD, the reference against render truth and against the single-tag poses, and the wrong builds' forms."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from isaac_ros_apriltag_amd import build, capi  # noqa: E402
import bundle_cases as bc  # noqa: E402
import pose_refine_ref as pr  # noqa: E402
import rigid_bundle_cases as rc  # noqa: E402
import rigid_bundle_ref as rr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "aux_c", "rigid_pose_driver.cpp")
INVALID_ARGUMENT = 1
NCODES36 = 587
_cache = {}


def scenes():
    """Every (name, records, bundle, intrinsics, skew) the GPU test solves."""
    if "scenes" not in _cache:
        out = []
        for n in rc.CUBE_FRAMES:
            slot = rc.CUBE_FRAMES.index(n)
            out += [("%s:%s" % (n, b["name"]), rc.cube_records(n), b, bc.INTR1[slot], bc.SKEW1[slot]) for b in rc.CUBE_BUNDLES]
        out.append(("turned", rc.turned_records(), rc.TURNED, bc.INTR1[0], 0.0))
        for n in bc.CONTENT:
            slot = bc.SLOTS[n][1]
            out.append((n, bc.content_records(n), rc.BUNDLE1, bc.INTR1[slot], bc.SKEW1[slot]))
        out += [("wave", bc.records72(), rc.FULL_WAVE, bc.INTR2, 0.0), ("ends", bc.records72(), rc.BOTH_ENDS, bc.INTR2, 0.0)]
        out += [("two:%s" % b["name"], bc.content_records("all_six"), b, bc.INTR1[0], 0.0) for b in rc.TWO]
        _cache["scenes"] = out
    return _cache["scenes"]


def moments():
    """Every M both chains of every scene form."""
    if "moments" not in _cache:
        ms = []
        for (_, recs, b, intr, skew) in scenes():
            rr.solve(recs, b, rc.FAMS, intr, skew, moments=ms)
        _cache["moments"] = ms
    return _cache["moments"]


# ---- the headers ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rigid_pose") / "librigid_pose.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", DRIVER, "-o", so])
    L = C.CDLL(so)
    D = C.POINTER(C.c_double)
    L.rigid_pose_probe.argtypes = [C.c_uint32] + [D] * 6 + [C.c_double] * 5 + [C.c_uint32, C.POINTER(capi.BundlePoseEx)]
    L.rigid_pose_probe.restype = C.c_int
    L.rigid_polar_probe.argtypes = [D, D]
    L.rigid_polar_probe.restype = C.c_int
    L.rigid_layout_probe.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(capi.BundleEx), D, C.c_uint32, C.POINTER(C.c_uint32)]
    L.rigid_layout_probe.restype = C.c_int
    L.rigid_pose_sizes.restype = C.c_uint32
    return L


def _layout(L, bundles, ncodes=(NCODES36,)):
    """(return code, the members' corners as a list of 4 x 3 lists) of rigid_layout.h on `bundles`."""
    arr = capi.bundles_ex(bundles)
    total = sum(len(b["members"]) for b in bundles)
    corners = (C.c_double * (12 * max(total, 1)))()
    n = C.c_uint32(0)
    rcode = L.rigid_layout_probe(len(ncodes), (C.c_uint32 * len(ncodes))(*ncodes), len(bundles), arr, corners, total, C.byref(n))
    vals = list(corners)
    return rcode, [[vals[12 * i + 3 * k:12 * i + 3 * k + 3] for k in range(4)] for i in range(n.value)]


def _flat(rows):
    v = [float(x) for r in rows for x in np.asarray(r, dtype=np.float64).reshape(-1)]
    return (C.c_double * max(len(v), 1))(*v)


def _header_solve(L, records, bundle, intrinsics, skew, bundle_index=0):
    """The record of rigid_pose.h, fed the layout of rigid_layout.h and what the reference reads of the records."""
    used, nskipped, pix, _, hom, mem = rr.inputs(records, bundle, rc.FAMS, intrinsics, skew)
    out = rr.zero_record(bundle_index, len(used), nskipped)
    if len(used) < int(bundle.get("min_tags", 1)):
        return out
    rcode, corners = _layout(L, [bundle])
    assert rcode == 0
    ids = [int(m[1]) for m in bundle["members"]]
    obj = [corners[ids.index(int(m[1]))] for _, m in used]
    o = capi.BundlePoseEx()
    intr = [rr.f32(v) for v in intrinsics]
    assert L.rigid_pose_probe(len(used), _flat(pix), _flat(obj), _flat([h[0] for h in hom]), _flat([h[1] for h in hom]), _flat([m[0] for m in mem]),
                              _flat([m[1] for m in mem]), intr[0], intr[1], intr[2], intr[3], rr.f32(skew), int(bundle["iterations"]), C.byref(o)) == 0
    out.update(status=int(o.status), seed=used[int(o.seed)][0], chosen=int(o.chosen), R=np.array(list(o.R)).reshape(3, 3), t=np.array(list(o.t)),
               err=float(o.err), sq_err_sum=float(o.sq_err_sum), R_alt=np.array(list(o.R_alt)).reshape(3, 3), t_alt=np.array(list(o.t_alt)),
               err_alt=float(o.err_alt), sq_err_sum_alt=float(o.sq_err_sum_alt))
    return out


def test_header_equals_the_reference(built, header):
    """csrc/rigid_layout.h and csrc/rigid_pose.h under g++ against the Python reference on every scene of the GPU test, every double as
    its 64 bits: the object points, then the record.  One and two hundred iterations on the cube corner as well."""
    errs = []
    for (name, recs, b, intr, skew) in scenes():
        rcode, corners = _layout(header, [b])
        assert rcode == 0
        want_corners = [rr.member_corners(m) for m in b["members"]]
        if not np.array_equal(rr.bits(corners), rr.bits(want_corners)):
            errs.append("%s: the object points differ" % name)
        want = rr.solve(recs, b, rc.FAMS, intr, skew)
        errs += rr.compare(_header_solve(header, recs, b, intr, skew), want, name + ": ")
    for it in (1, 2, 200):
        b = dict(rc.CUBE, iterations=it)
        errs += rr.compare(_header_solve(header, rc.cube_records("cube_a"), b, bc.INTR1[0], 0.0),
                           rr.solve(rc.cube_records("cube_a"), b, rc.FAMS, bc.INTR1[0], 0.0), "cube_a, %d iterations: " % it)
    print(errs[:10])
    assert not errs
    # the rotation step alone on every M, and where the leading singular value vanishes
    for M in moments():
        Rn = (C.c_double * 9)()
        ok = header.rigid_polar_probe((C.c_double * 9)(*M), Rn)
        want, pos = rr.polar(M)
        assert bool(ok) == pos and np.array_equal(rr.bits(list(Rn)), rr.bits(want))
    assert header.rigid_polar_probe((C.c_double * 9)(*([0.0] * 9)), (C.c_double * 9)()) == 0 and not rr.polar([0.0] * 9)[1]


def test_header_under_asan_ubsan(tmp_path):
    """The same headers in a program of its own (the driver's main), built with -fsanitize=address,undefined and run here."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void){return 0;}\n")
    if not shutil.which("g++") or subprocess.run(["gcc"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode:
        pytest.skip("no sanitizer runtime for g++")
    exe = str(tmp_path / "rigid_pose_san")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-DRIGID_POSE_MAIN"] + san + [DRIVER, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])


# ---- the layout's refusals -------------------------------------------------------------------------------------------------------------------
_OK_MEMBER = (0, 4, rc.I3, (0.1, 0.2, 0.3), 0.1)
_OK = {"name": "ok", "iterations": 50, "members": [_OK_MEMBER]}
_TILTED = np.array([[1.0, 2e-6, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])   # |R R^T - I| = 2e-6
_NEARLY = np.array([[1.0, 5e-7, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])   # 5e-7: within the bound, taken as it stands
_REFUSED = {
    "family_index": [dict(_OK, members=[(1, 4, rc.I3, (0, 0, 0), 0.1)])],
    "id": [dict(_OK, members=[(0, NCODES36, rc.I3, (0, 0, 0), 0.1)])],
    "zero_size": [dict(_OK, members=[(0, 4, rc.I3, (0, 0, 0), 0.0)])],
    "nan_size": [dict(_OK, members=[(0, 4, rc.I3, (0, 0, 0), float("nan"))])],
    "nan_t": [dict(_OK, members=[(0, 4, rc.I3, (0, float("nan"), 0), 0.1)])],
    "inf_R": [dict(_OK, members=[(0, 4, np.diag([1.0, float("inf"), 1.0]), (0, 0, 0), 0.1)])],
    "not_orthonormal": [dict(_OK, members=[(0, 4, _TILTED, (0, 0, 0), 0.1)])],
    "scaled_R": [dict(_OK, members=[(0, 4, 1.001 * rc.I3, (0, 0, 0), 0.1)])],
    "reflection": [dict(_OK, members=[(0, 4, np.diag([1.0, 1.0, -1.0]), (0, 0, 0), 0.1)])],
    "min_tags_0": [dict(_OK, min_tags=0)],
    "iterations_0": [dict(_OK, iterations=0)],
    "iterations_201": [dict(_OK, iterations=201)],
    "named_twice": [_OK, dict(_OK, name="again")],
    "named_twice_within": [dict(_OK, members=[_OK_MEMBER, _OK_MEMBER])],
    "nine_bundles": [dict(_OK, members=[(0, i, rc.I3, (0, 0, 0), 0.1)]) for i in range(9)],
    "65_members": [dict(_OK, members=[(0, i, rc.I3, (0, 0, 0), 0.1) for i in range(65)])],
    "no_members": [dict(_OK, members=[])],
}


@pytest.mark.parametrize("case", sorted(_REFUSED))
def test_layout_refuses(header, case):
    assert _layout(header, _REFUSED[case])[0] == INVALID_ARGUMENT
    if case in ("not_orthonormal", "scaled_R", "reflection"):   # (the reference states the same bound)
        assert not rr.is_rotation(_REFUSED[case][0]["members"][0][2]) and rr.is_rotation(_NEARLY)


def test_layout_accepts(header):
    """What is within the bounds: 64 members, 8 bundles, 200 iterations, a rotation within 1e-6 of orthonormal (taken as it stands: the
    object points carry its entries), the empty layout; a name without terminator and null pointers are refused."""
    assert _layout(header, [dict(_OK, iterations=200, members=[(0, i, rc.I3, (0, 0, 0), 0.1) for i in range(64)])])[0] == 0
    assert _layout(header, [dict(_OK, members=[(0, i, rc.I3, (0, 0, 0), 0.1)]) for i in range(8)])[0] == 0
    rcode, corners = _layout(header, [dict(_OK, members=[(0, 4, _NEARLY, (0, 0, 0), 0.1)])])
    assert rcode == 0 and np.array_equal(rr.bits(corners[0]), rr.bits(rr.member_corners((0, 4, _NEARLY, (0, 0, 0), 0.1))))
    assert corners[0][0][0] != -0.05   # (the 5e-7 is in the points)
    n = C.c_uint32(7)
    assert header.rigid_layout_probe(1, (C.c_uint32 * 1)(NCODES36), 0, None, None, 0, C.byref(n)) == 0 and n.value == 0
    assert header.rigid_layout_probe(1, (C.c_uint32 * 1)(NCODES36), 1, None, None, 0, C.byref(n)) == INVALID_ARGUMENT
    arr = capi.bundles_ex([_OK])
    C.memset(C.addressof(arr[0]) + capi.BundleEx.name.offset, ord("x"), 32)
    assert header.rigid_layout_probe(1, (C.c_uint32 * 1)(NCODES36), 1, arr, (C.c_double * 12)(), 1, C.byref(n)) == INVALID_ARGUMENT
    arr = capi.bundles_ex([_OK])
    arr[0].members = None
    assert header.rigid_layout_probe(1, (C.c_uint32 * 1)(NCODES36), 1, arr, (C.c_double * 12)(), 1, C.byref(n)) == INVALID_ARGUMENT


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(tmp_path, header):
    structs = {"amdAprilTagsBundleMemberEx_t": (capi.BundleMemberEx, ("family_index", "id", "R", "t", "size")),
               "amdAprilTagsBundleEx_t": (capi.BundleEx, ("members", "nmembers", "max_hamming", "min_decision_margin", "min_tags", "iterations", "name")),
               "amdAprilTagsBundlePoseEx_t": (capi.BundlePoseEx, ("bundle", "status", "ntags", "nskipped", "seed", "chosen", "R", "t", "err", "sq_err_sum",
                                                                  "R_alt", "t_alt", "err_alt", "sq_err_sum_alt"))}
    lines, want = [], []
    for cname, (cls, names) in sorted(structs.items()):
        lines += ['printf("%%zu ", sizeof(%s));' % cname] + ['printf("%%zu ", offsetof(%s, %s));' % (cname, n) for n in names]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in names]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "apriltag_amd.h"\nint main(void){ %s return 0; }\n' % " ".join(lines))
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert [int(v) for v in subprocess.check_output([exe]).decode().split()] == want
    assert header.rigid_pose_sizes(0) == C.sizeof(capi.BundlePoseEx) == 248
    assert header.rigid_pose_sizes(1) == C.sizeof(capi.BundleEx) and header.rigid_pose_sizes(2) == C.sizeof(capi.BundleMemberEx)
    assert header.rigid_pose_sizes(3) == capi.MAX_RIGID_BUNDLE_MEMBERS == rr.SLOTS == 64 and header.rigid_pose_sizes(4) == rr.SWEEPS
    assert (capi.BUNDLE_SOLVED, capi.BUNDLE_TOO_FEW_TAGS, capi.BUNDLE_DEGENERATE) == (rr.SOLVED, rr.TOO_FEW_TAGS, rr.DEGENERATE) == (0, 1, 3)
    hdr = open(os.path.join(ROOT, "include", "apriltag_amd.h")).read()
    for text in ("#define AMDAT_BUNDLE_DEGENERATE 3u", "#define AMDAT_MAX_RIGID_BUNDLE_MEMBERS 64u", "#define AMDAT_CONFIG_LAYOUT_VERSION 3",
                 "max |R R^T - I| > 1e-6"):
        assert text in hdr
    assert "amdAprilTagsSetBundlesEx" in capi.EXPORTS and "amdAprilTagsGetBundlePosesEx" in capi.EXPORTS


def test_library_refuses_without_a_device(built):
    """amdAprilTagsSetBundlesEx / GetBundlePosesEx: the null handle, before any HIP call."""
    if not os.path.exists(capi.LIB_PATH):
        build.build_amd()
    L = capi.lib()
    rec = capi.BundlePoseEx()
    assert L.amdAprilTagsSetBundlesEx(None, 0, None) == INVALID_ARGUMENT
    assert L.amdAprilTagsSetBundlesEx(None, 1, capi.bundles_ex([_OK])) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetBundlePosesEx(None, C.byref(rec), 1) == INVALID_ARGUMENT


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def _svd_rotation(M):
    U, s, Vt = np.linalg.svd(np.array(M).reshape(3, 3))
    return U @ np.diag([1.0, 1.0, float(np.sign(np.linalg.det(U @ Vt)))]) @ Vt, s


def test_rotation_step_against_numpy_svd(built):
    """R+ of every M of every scene against U diag(1, 1, det(U V^T)) V^T of numpy.linalg.svd, per sweep count: the table of DESIGN.md
    section 7f.  The bound: at rg_polar's count the difference is rounding -- R+ is assembled from a few dozen products of entries of
    size at most one, each within 2^-53 relative, and the eigenvectors of S = M^T M carry cond-amplified rounding, the second singular
    value being no smaller than 0.1 of the first on these scenes: below 64 * 10 * 2^-53 = 7.2e-14; R+^T R+ - I, which no
    conditioning enters, below 32 * 2^-53 = 3.6e-15.  One sweep fewer gives the same figures, two fewer do not."""
    ms = moments()
    svd = [_svd_rotation(M) for M in ms]
    assert min(s[1] / s[0] for _, s in svd) > 0.1 and min(s[2] / s[0] for _, s in svd) < 1e-12   # (coplanar sets are among them)
    table = {}
    for sweeps in range(1, 8):
        d = o = 0.0
        for M, (Rs, _) in zip(ms, svd):
            R, pos = rr.polar(M, sweeps)
            R = np.array(R).reshape(3, 3)
            assert pos and np.linalg.det(R) > 0.99
            d = max(d, float(np.abs(R - Rs).max()))
            o = max(o, float(np.abs(R.T @ R - np.eye(3)).max()))
        table[sweeps] = (d, o)
        print("sweeps %d: max |R+ - R_svd| %.3e, max |R+^T R+ - I| %.3e over %d matrices" % (sweeps, d, o, len(ms)))
    assert table[rr.SWEEPS][0] < 7.2e-14 and table[rr.SWEEPS][1] < 3.6e-15
    assert all(table[k][0] < 7.2e-14 and table[k][1] < 3.6e-15 for k in (rr.SWEEPS - 1, rr.SWEEPS + 1)) and table[rr.SWEEPS - 2][0] > 7.2e-14


def test_reference_against_render_truth(built):
    """The cube corner under the camera it was rendered with (slot 0): the bundle's rotation and translation error against the median
    error of section 7e's chosen single-tag poses of the same frame, each composed with its member's inverse -- what the parent commit
    can do per tag.  The bundle must be no worse in either."""
    recs = rc.cube_records("cube_a")
    Rt, tt = rc.CUBE_POSES["cube_a"]
    sol = rc.cube_solved("cube_a")[0]
    assert sol["status"] == rr.SOLVED and sol["ntags"] == 12
    eb = rc.pose_errors(sol["R"], sol["t"], Rt, tt)
    by_id = {int(m[1]): m for m in rc.CUBE_MEMBERS}
    single = []
    for r in recs:
        m = by_id[int(r["id"])]
        Rh, th = rr.po.pose_from_homography(r["H"], *[rr.f32(v) for v in bc.INTR1[0]], float(m[4]), 0.0)
        ref = pr.refine(r["p"], bc.INTR1[0], 0.0, m[4], Rh, th, rr.ITERATIONS)
        Rb = ref["R"] @ np.asarray(m[2]).T
        single.append(rc.pose_errors(Rb, ref["t"] - Rb @ np.asarray(m[3]), Rt, tt))
    med = (float(np.median([e[0] for e in single])), float(np.median([e[1] for e in single])))
    print("cube corner against render truth: bundle %.4f degrees, %.3f mm; median of the 12 single-tag poses %.4f degrees, %.3f mm"
          % (eb[0], 1e3 * eb[1], med[0], 1e3 * med[1]))
    assert eb[0] <= med[0] and eb[1] <= med[1]
    # a non-coplanar set has one minimum: both chains end in it; one face alone keeps the planar ambiguity
    assert pr.rot_angle_deg(sol["R"], sol["R_alt"]) < 1e-3
    face = rc.cube_solved("one_face")[0]
    assert face["status"] == rr.SOLVED and face["ntags"] == 4 and pr.rot_angle_deg(face["R"], face["R_alt"]) > 20.0 and face["err"] < face["err_alt"]
    assert rc.pose_errors(face["R"], face["t"], *rc.FACE_POSE)[0] < 2.0


def test_gpu_preconditions_on_the_oracle_side(built):
    """What tests/test_rigid_bundles_gpu.py relies on: which tags each frame holds and which slots they fill, the seeds, the statuses;
    the wrong builds' forms of the definition differ from the product form exactly on the cases they must fail; hooks 19 and 20 are
    registered."""
    assert [[r["id"] for r in rc.cube_records(n)] for n in rc.CUBE_FRAMES] == [list(range(12)), [0, 1, 2, 3, rc.LONE_ID], list(range(12))]
    assert [(s[0]["status"], s[0]["ntags"], s[1]["status"], s[1]["ntags"]) for s in map(rc.cube_solved, rc.CUBE_FRAMES)] == \
        [(0, 12, 1, 0), (0, 4, 0, 1), (0, 12, 1, 0)]
    lone = rc.cube_solved("one_face")[1]
    assert lone["seed"] == 4   # (the lone tag's record is the frame's last)
    assert [r["id"] for r in rc.turned_records()] == list(range(6)) and rc.turned_solved()["ntags"] == 6
    assert rc.pose_errors(rc.turned_solved()["R"], rc.turned_solved()["t"], bc.R1, bc.T1)[0] < 0.5
    wave, ends = rc.solved72("wave"), rc.solved72("ends")
    assert len(bc.records72()) == 72 and (wave["status"], wave["ntags"], wave["nskipped"]) == (0, 64, 0) and (ends["status"], ends["ntags"]) == (0, 12)
    used, _ = rr.used_slots(bc.records72(), rc.BOTH_ENDS, rc.FAMS)
    assert min(i for i, _ in used) < 64 <= max(i for i, _ in used)   # both chunks of the canonical order
    assert rc.content_solved("no_tags")["status"] == rr.TOO_FEW_TAGS and rc.content_solved("duplicate")["nskipped"] == 2
    assert rc.content_solved("hamming")["nskipped"] == 1 and rc.content_solved("painted_over")["ntags"] == 5

    def differs(name, recs, b, intr, skew, **form):
        return bool(rr.compare(rr.solve(recs, b, rc.FAMS, intr, skew, **form), rr.solve(recs, b, rc.FAMS, intr, skew)))
    for (name, recs, b, intr, skew) in scenes():
        ntags = rr.solve(recs, b, rc.FAMS, intr, skew)["ntags"]
        turned = any(not np.array_equal(np.asarray(m[2]), rc.I3) for m in b["members"])
        assert differs(name, recs, b, intr, skew, member_rotation=False) == (turned and ntags >= 1), name   # mutant 19
        assert differs(name, recs, b, intr, skew, npts_of=lambda n: 4.0) == (ntags >= 2), name              # mutant 20
    hooks = open(os.path.join(ROOT, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    assert 19 in build.MUTANTS and 20 in build.MUTANTS and "AMDAT_MUTATE == 19" in hooks and "AMDAT_MUTATE == 20" in hooks
