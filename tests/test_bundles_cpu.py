"""CPU checks of the board pose of a tag bundle (amdAprilTagsSetBundles): the Python reference tests/bundle_ref.py
against an independent least-squares formulation and against analytic truth on rendered boards; the host half of the library
(csrc/bundle_layout.h: refusals, normalisation constants, lookup table), also under the host sanitizers in a program of its own; and the
struct layouts of capi.py against the header."""
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
import bundle_ref as br  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "aux_c", "bundle_layout_driver.cpp")
FAMS = list(bc.FAM)
INVALID_ARGUMENT = 1


# ---- the reference against an independent formulation ----------------------------------------------------------------------------------
def _lstsq_cases():
    two = dict(bc.BUNDLE1, members=bc.MEMBERS1[:2])
    return {"six": (bc.content_records("all_six"), bc.BUNDLE1, bc.INTR1[0], bc.SKEW1[0]),
            "five-skew": (bc.content_records("painted_over"), bc.BUNDLE1, bc.INTR1[1], bc.SKEW1[1]),
            "seventy-two": (bc.records72(), bc.BUNDLE2, bc.INTR2, 0.0),
            "one-tag": (bc.content_records("non_member"), bc.BUNDLES3[2], bc.INTR1[2], bc.SKEW1[2]),
            "two-tags": (bc.content_records("non_member"), two, bc.INTR1[2], bc.SKEW1[2])}


@pytest.mark.parametrize("name", ("six", "five-skew", "seventy-two", "one-tag", "two-tags"))
def test_reference_against_lstsq(built, name):
    """numpy.linalg.lstsq on the stacked rows, in the same normalised coordinates: the eight h agree within 64 cond(M) 2^-53 relative (the
    forward error of a backward-stable solve of the normal equations, cond(M) = cond(rows)^2 computed here, with 64 for the constants of
    the 8 x 8 elimination)."""
    recs, bundle, intr, skew = _lstsq_cases()[name]
    out = br.solve(recs, bundle, FAMS, intr, skew)
    assert out["status"] == br.SOLVED
    norm = br.normalisation(bundle["members"])
    cls = br.classify(recs, bundle, FAMS)
    used = [(c[0], recs[i]["p"]) for i, c in enumerate(cls) if c is not None and c[1]]
    rows = np.array([r for m, p in used for r in br.rows_of(m, p, norm, tuple(br.f32(v) for v in intr), br.f32(skew))])
    assert rows.shape == (8 * out["ntags"], 9)
    h = np.linalg.lstsq(rows[:, :8], rows[:, 8], rcond=None)[0]
    cond = float(np.linalg.cond(rows[:, :8].T @ rows[:, :8]))
    rel = float(np.linalg.norm(np.array(out["h"][:8]) - h) / np.linalg.norm(h))
    print("%s: %d tags, cond(M) %.3g, relative difference %.3g, bound %.3g" % (name, out["ntags"], cond, rel, 64 * cond * 2.0 ** -53))
    assert rel <= 64 * cond * 2.0 ** -53


# ---- the reference against analytic truth ----------------------------------------------------------------------------------------------
# observed here: board (rotation: max abs entry, translation: max abs component in metres)
TRUTH = {"six": (7.9e-4, 1.23e-4), "seventy-two": (4.6e-5, 3.4e-6)}


@pytest.mark.parametrize("name", sorted(TRUTH))
def test_reference_against_truth(built, name):
    """Rendered boards detected by the oracle under the camera they were rendered with: the board pose is no further from the truth than
    the median single-tag pose of the same frame, in rotation and in translation, and within twice the error observed when this test was
    written (renderer seeds)."""
    if name == "six":
        recs, bundle, intr, R, T, members = bc.oracle_records(bc.content_frame("all_six"), bc.INTR1[0]), bc.BUNDLE1, bc.INTR1[0], bc.R1, bc.T1, bc.MEMBERS1
    else:
        recs, bundle, intr, R, T, members = bc.records72(), bc.BUNDLE2, bc.INTR2, bc.R2, bc.T2, bc.MEMBERS2
    out = br.solve(recs, bundle, FAMS, intr)
    assert out["status"] == br.SOLVED and out["ntags"] == len(members) and out["nskipped"] == 0
    pos = {m[1]: np.array([m[2], m[3], 0.0]) for m in members}
    tag_r = [br.rot_err(r["R"], R) for r in recs]
    tag_t = [float(np.abs(r["t"] - (T + R @ pos[r["id"]])).max()) for r in recs]
    board_r, board_t = br.rot_err(out["R"], R), float(np.abs(out["t"] - T).max())
    print("%s: board rotation %.3g translation %.3g m; median tag rotation %.3g translation %.3g m; rms %.3g px"
          % (name, board_r, board_t, np.median(tag_r), np.median(tag_t), br.rms(out)))
    assert board_r <= np.median(tag_r) and board_t <= np.median(tag_t)
    assert board_r <= 2 * TRUTH[name][0] and board_t <= 2 * TRUTH[name][1]
    assert br.rms(out) < 0.25   # corners to a fraction of a pixel


def test_reference_gates_and_duplicates(built):
    """What the content cases of the GPU test rely on: the oracle's records hold the duplicate pair contiguously, the painted bit decodes
    with hamming 1, and the reference counts them as skipped."""
    want = {"all_six": (br.SOLVED, 6, 0), "painted_over": (br.SOLVED, 5, 0), "non_member": (br.SOLVED, 6, 0), "duplicate": (br.SOLVED, 5, 2),
            "hamming": (br.SOLVED, 5, 1), "no_tags": (br.TOO_FEW_TAGS, 0, 0)}
    for name in bc.CONTENT:
        slot = bc.SLOTS[name][1]
        out = br.solve(bc.content_records(name), bc.BUNDLE1, FAMS, bc.INTR1[slot], bc.SKEW1[slot])
        assert (out["status"], out["ntags"], out["nskipped"]) == want[name], name
        if out["status"] != br.SOLVED:
            assert not out["R"].any() and not out["t"].any() and out["sq_err_sum"] == 0.0
    ids = [r["id"] for r in bc.content_records("duplicate")]
    assert ids == [0, 1, 1, 2, 3, 4, 5]
    assert [r["hamming"] for r in bc.content_records("hamming")] == [0, 0, 1, 0, 0, 0]
    assert len(bc.records72()) == 72 and sorted(r["id"] for r in bc.records72()) == list(range(72))
    # the wrong builds of the GPU suite change values: corners in the order p[3 - k] give another pose
    a = br.solve(bc.content_records("all_six"), bc.BUNDLE1, FAMS, bc.INTR1[0])
    b = br.solve(bc.content_records("all_six"), bc.BUNDLE1, FAMS, bc.INTR1[0], corner_of=lambda k: 3 - k)
    assert br.compare(b, a)
    hooks = open(os.path.join(ROOT, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    assert 15 in build.MUTANTS and 16 in build.MUTANTS and "AMDAT_MUTATE == 15" in hooks and "AMDAT_MUTATE == 16" in hooks


# ---- the host half of the library ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bundle_layout") / "libbundle_layout.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", DRIVER, "-o", so])
    L = C.CDLL(so)
    L.bundle_layout_probe.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(capi.Bundle), C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_uint16), C.c_uint32, C.POINTER(C.c_uint32)]
    L.bundle_layout_sizes.restype = C.c_uint32
    ncodes = (C.c_uint32 * 2)(587, 35)

    def probe(specs, raw=None, nbundles=None):
        arr = raw if raw is not None else capi.bundles(specs)
        n = nbundles if nbundles is not None else (len(arr) if arr is not None else 0)
        norm, mem, table, counts = (C.c_double * 24)(), (C.c_double * 4096)(), (C.c_uint16 * 622)(), (C.c_uint32 * 2)()
        rc = L.bundle_layout_probe(2, ncodes, n, arr, norm, mem, table, 622, counts)
        if rc:
            return rc, None
        nb = n
        return 0, {"norm": [tuple(norm[3 * b:3 * b + 3]) for b in range(nb)], "members": [tuple(mem[4 * m:4 * m + 4]) for m in range(counts[0])],
                   "table": list(table[:counts[1]])}
    probe.lib = L
    return probe


def test_layout_constants_and_table(layout):
    """mx, my, sc equal the reference's, bit for bit; the table holds 1 + the member's index at fam_base[family] + id and 0 elsewhere."""
    second = {"name": "b", "members": [(1, 3, 0.25, -1.5, 0.1), (1, 0, 0.3, 0.7, 0.2), (0, 586, 1e3, 0.1, 0.3)], "min_tags": 2}
    rc, got = layout([bc.BUNDLE1, dict(bc.BUNDLE2, members=[(0, 100 + m[1]) + m[2:] for m in bc.MEMBERS2]), second])
    assert rc == 0
    specs = [bc.MEMBERS1, [(0, 100 + m[1]) + m[2:] for m in bc.MEMBERS2], second["members"]]
    for b, members in enumerate(specs):
        assert got["norm"][b] == br.normalisation(members)
    flat = [(b, m) for b, members in enumerate(specs) for m in members]
    assert got["members"] == [(m[2], m[3], m[4] / 2.0, float(b)) for b, m in flat]
    want = [0] * (587 + 35)
    for i, (b, m) in enumerate(flat):
        want[(0 if m[0] == 0 else 587) + m[1]] = i + 1
    assert got["table"] == want and len(got["table"]) == 622
    assert layout(None) == (0, {"norm": [], "members": [], "table": [0] * 622})


def test_layout_refusals(layout):
    """Everything amdAprilTagsSetBundles refuses before it touches the device."""
    ok = {"name": "ok", "members": [(0, 4, 1.0, 1.0, 0.1), (1, 5, 0.0, 0.0, 0.1)]}
    assert layout([ok])[0] == 0
    inf, nan = float("inf"), float("nan")
    for bad in ((2, 5, 0, 0, 0.1), (0, 587, 0, 0, 0.1), (1, 35, 0, 0, 0.1), (0, 5, inf, 0, 0.1), (0, 5, 0, nan, 0.1), (0, 5, 0, 0, 0.0),
                (0, 5, 0, 0, -0.1), (0, 5, 0, 0, inf), (0, 5, 0, 0, nan), (0, 4, 0, 0, 0.1)):   # (the last: named twice within the bundle)
        assert layout([dict(ok, members=[ok["members"][0], bad])])[0] == INVALID_ARGUMENT, bad
    assert layout([ok, dict(ok, name="again")])[0] == INVALID_ARGUMENT       # named twice across bundles
    assert layout([dict(ok, min_tags=0)])[0] == INVALID_ARGUMENT
    many = [{"name": "b%d" % i, "members": [(0, i, 0.0, 0.0, 0.1)]} for i in range(9)]
    assert layout(many[:8])[0] == 0 and layout(many)[0] == INVALID_ARGUMENT    # at most 8 bundles
    full = [(0, i, 0.1 * i, 0.0, 0.05) for i in range(587)] + [(1, i, 0.1 * i, 1.0, 0.05) for i in range(35)]
    assert layout([{"name": "full", "members": full}])[0] == 0
    arr = capi.bundles([ok])
    arr[0].nmembers = 1025                                                      # more than 1024 members in all
    assert layout(None, raw=arr)[0] == INVALID_ARGUMENT
    arr = capi.bundles([ok])
    arr[0].nmembers = 0
    assert layout(None, raw=arr)[0] == INVALID_ARGUMENT
    arr = capi.bundles([ok])
    arr[0].members = None
    assert layout(None, raw=arr)[0] == INVALID_ARGUMENT
    arr = capi.bundles([ok])
    C.memset(C.addressof(arr[0]) + capi.Bundle.name.offset, ord("n"), 32)      # a name without terminator
    assert layout(None, raw=arr)[0] == INVALID_ARGUMENT
    assert layout(None, raw=None, nbundles=1)[0] == INVALID_ARGUMENT           # null bundles with nbundles > 0
    with pytest.raises(ValueError):
        capi.bundles([dict(ok, name="n" * 32)])


def test_layout_under_asan_ubsan(tmp_path):
    """The same host code in a program of its own (the driver's main), built with -fsanitize=address,undefined and run here."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void){return 0;}\n")
    if not shutil.which("g++") or subprocess.run(["gcc"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode:
        pytest.skip("no sanitizer runtime for g++")
    exe = str(tmp_path / "bundle_layout_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-DBUNDLE_LAYOUT_MAIN"] + san + [DRIVER, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])


# ---- struct layouts ----------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_header(tmp_path, layout):
    fields = {"amdAprilTagsBundleMember_t": (capi.BundleMember, ("family_index", "id", "x", "y", "size")),
              "amdAprilTagsBundle_t": (capi.Bundle, ("members", "nmembers", "max_hamming", "min_decision_margin", "min_tags", "name")),
              "amdAprilTagsBundlePose_t": (capi.BundlePose, ("bundle", "status", "ntags", "nskipped", "R", "t", "sq_err_sum"))}
    lines = []
    for t, (_, names) in fields.items():
        lines.append('printf("%%zu", sizeof(%s));' % t)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (t, n) for n in names]
        lines.append('printf("\\n");')
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "apriltag_amd.h"\nint main(void){ %s return 0; }\n' % " ".join(lines))
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [[int(v) for v in l.split()] for l in subprocess.check_output([exe]).decode().splitlines()]
    for row, (t, (cls, names)) in zip(out, fields.items()):
        assert row == [C.sizeof(cls)] + [getattr(cls, n).offset for n in names], t
    assert [layout.lib.bundle_layout_sizes(i) for i in range(3)] == [C.sizeof(capi.BundleMember), C.sizeof(capi.Bundle), C.sizeof(capi.BundlePose)]
    assert layout.lib.bundle_layout_sizes(3) == C.sizeof(capi.BundlePose) + 8   # the pinned record: the stamp behind the public one
    assert (capi.BUNDLE_SOLVED, capi.BUNDLE_TOO_FEW_TAGS, capi.BUNDLE_SINGULAR, capi.MAX_BUNDLES, capi.MAX_BUNDLE_MEMBERS) == (0, 1, 2, 8, 1024)
    hdr = open(os.path.join(ROOT, "include", "apriltag_amd.h")).read()
    for text in ("#define AMDAT_BUNDLE_SOLVED 0u", "#define AMDAT_BUNDLE_TOO_FEW_TAGS 1u", "#define AMDAT_BUNDLE_SINGULAR 2u",
                 "#define AMDAT_MAX_BUNDLES 8u", "#define AMDAT_MAX_BUNDLE_MEMBERS 1024u"):
        assert text in hdr


def test_library_refuses_without_a_device(built):
    """amdAprilTagsSetBundles / GetBundlePoses: the null handle, before any HIP call."""
    if not os.path.exists(capi.LIB_PATH):
        build.build_amd()
    L = capi.lib()
    assert L.amdAprilTagsSetBundles(None, 0, None) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetBundlePoses(None, None, 0) == INVALID_ARGUMENT
