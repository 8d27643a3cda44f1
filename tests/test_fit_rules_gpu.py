"""The quad fit's floating-point rules on the frames of tests/fit_rule_frames.py: the box and border-direction tests, the cut to
max_nmaxima corners at each of its four sites, and the determinant, area, angle and winding tests of k_quad_finish are met here by
construction, each with a twin on the other side of the rule.  Every frame goes through parity_util's comparison -- all stages and quads
bit for bit, on both launch sets, alone and in one submission with the frames of its size, under the family and decimate it was built
for -- and then the census of tests/test_fit_rule_frames_cpu.py is repeated on the library's own cluster and quad lists: the quads named
there exist, and the clusters named as dropped have none.  Wrong builds 37 .. 45 (csrc/tools_hooks.h) show that each case fails where
its rule is broken."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
import fit_rule_frames as fr  # noqa: E402
import parity_util as pu  # noqa: E402

PATHS = ("latency", "throughput")
_REGISTERED = []   # the reversed-border family, once per process


def _submit(names, path):
    """One submission of the frames `names` -- one family, decimate and size -- on launch set `path`: every stage, quad and record of
    every frame against the oracle, then per frame the census on the library's DBG_CLUSTERS and DBG_QUADS."""
    fam, dec, _ = fr.FRAMES[names[0]]
    imgs = [fr.frame(n) for n in names]
    assert all(fr.FRAMES[n][:2] == (fam, dec) and fr.frame(n).shape == imgs[0].shape for n in names)
    if fam == fr.REVERSED and not _REGISTERED:
        capi.register_family_ex(*fr.reversed_family_args())
        _REGISTERED.append(fam)
    h, w = imgs[0].shape
    K = synth.default_K(w, h)
    det = AprilTagDetector(w, h, families=(fam,), decimate=dec, intrinsics=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), max_batch=len(imgs))
    try:
        det.set_submission_path(path)
        g = det.detect_batch_ex(torch.from_numpy(np.stack(imgs)).cuda(), max_dets=64)
        errs, lists = [], []
        for i, (n, img) in enumerate(zip(names, imgs)):
            e, odets = pu.compare_stages(det, i, img, (fr.oracle_family(fam),), K, dec)
            e += pu.compare_detections(g[i], odets)
            errs += ["%s: %s" % (n, x) for x in e]
            lists.append((det.debug(i, capi.DBG_CLUSTERS), det.debug(i, capi.DBG_QUADS)))
    finally:
        det.close()
    assert not errs, errs[:4]
    for n, (cl, q) in zip(names, lists):
        kept, dropped = fr.expectation(n)
        assert {int(k) for k in q["key"]} == kept and {int(k) for k in cl["key"]} == kept | dropped, n


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(fr.FRAMES))
def test_frame_alone(built, name, path):
    """exits_*: a straight edge, a square cut by the frame's corner, bars with two and with four maxima, darts at four turns, rhombi
    and kites of 6 .. 14 degrees, shallow vertices.  area_*: rectangles whose Heron area straddles 0.95 w^2 for w = 8, 7 and 6, and the
    decimate-2 frame no cluster leaves by area.  border_*: one frame under a reversed-border family alone and under tag36h11.  cut_*: a
    kept quad whose weakest corner is the tenth largest maximum, once per site of the cut; cuttwin_*: a kept quad that is not the one the
    search over all maxima would choose, once per site; the multi-wave ones also 2049 wide."""
    _submit([name], path)


_GROUPS = {"%s_d%d_%dx%d" % k: v for k, v in fr.groups().items() if len(v) > 1}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("group", sorted(_GROUPS))
def test_frames_of_one_size_in_one_submission(built, group, path):
    _submit(_GROUPS[group], path)


# ---- nine wrong builds ----------------------------------------------------------------------------------------------------------------------------
def _both(*names):
    """The ids of test_frame_alone for `names` on both launch sets."""
    return tuple("test_frame_alone[%s-%s]" % (n, p) for n in names for p in PATHS)


_CUT_ALL = ("cut_small", "cut_wave", "cut_regs", "cut_regs_wide", "cut_lds", "cut_lds_wide")
_WRONG_BUILDS = {
    # 37: the area limit as 1.0 w^2: the kept rectangles under w^2 go, the twins at or above w^2 stay
    37: {"select": "test_frame_alone and area_",
         "must_fail": _both("area_tag36h11_window", "area_tag25h9_window", "area_tag16h5_window"),
         "must_pass": _both("area_tag36h11_above", "area_tag25h9_above", "area_tag16h5_above", "area_dec2")},
    # 38: no cos_dtheta < -cos_critical_rad: the kites with a tip under 10 degrees are kept; a sharp rhombus still fails the upper test
    # or the corner search, a dart the winding term
    38: {"select": "test_frame_alone and (exits_kites or exits_darts or exits_rhombi)",
         "must_fail": _both("exits_kites_dropped"),
         "must_pass": _both("exits_darts", "exits_kites_kept", "exits_rhombi_a", "exits_rhombi_b")},
    # 39: no winding term: the darts are kept
    39: {"select": "test_frame_alone and (exits_kites or exits_darts or exits_rhombi)",
         "must_fail": _both("exits_darts"),
         "must_pass": _both("exits_kites_dropped", "exits_kites_kept", "exits_rhombi_a", "exits_rhombi_b")},
    # 40: fit_border_unwanted without its normal_border statement: the reversed-only handle keeps the normal quads too
    40: {"select": "test_frame_alone and border_", "must_fail": _both("border_reversed_only"), "must_pass": _both("border_tag36h11")},
    # 41 .. 44: the cut keeps nine, one site each: k_fit_small (the throughput set's fit of clusters up to 128 points), k_fit_quads with
    # up to 64 maxima, up to 64 * FQ_SEL_REGS, above
    41: {"select": "test_frame_alone and cut_", "must_fail": ("test_frame_alone[cut_small-throughput]",),
         "must_pass": ("test_frame_alone[cut_small-latency]",) + _both(*_CUT_ALL[1:])},
    42: {"select": "test_frame_alone and cut_", "must_fail": ("test_frame_alone[cut_small-latency]",) + _both("cut_wave"),
         "must_pass": ("test_frame_alone[cut_small-throughput]",) + _both(*_CUT_ALL[2:])},
    43: {"select": "test_frame_alone and cut_", "must_fail": _both("cut_regs", "cut_regs_wide"),
         "must_pass": _both("cut_small", "cut_wave", "cut_lds", "cut_lds_wide")},
    44: {"select": "test_frame_alone and cut_", "must_fail": _both("cut_lds", "cut_lds_wide"),
         "must_pass": _both("cut_small", "cut_wave", "cut_regs", "cut_regs_wide")},
    # 45: the corner search without its dot test: cut_wave's kept quad is the one that test decides; in the others it removes no winner
    45: {"select": "test_frame_alone and cut_", "must_fail": _both("cut_wave"),
         "must_pass": _both("cut_small", "cut_regs", "cut_regs_wide", "cut_lds", "cut_lds_wide")},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_fit_rule_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut37.so .. _mut45.so (csrc/tools_hooks.h, AMDAT_MUTATE): a narrow selection of this file's cases, in a process of
    its own, must FAIL on the wrong build where its error lives -- the quad list differs -- and pass on the twin where it cannot show; all
    of it passes on the product library."""
    import subprocess
    from isaac_ros_apriltag_amd import build as bld
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(bld.lib_mutant(mutant)):
        bld.build_mutants()
    spec = _WRONG_BUILDS[mutant]

    def run(lib):
        env = dict(os.environ)
        env.pop("AMDAT_LIB", None)
        if lib:
            env["AMDAT_LIB"] = lib
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", os.path.basename(__file__)),
                              "-m", "gpu", "-q", "-rA", "-p", "no:cacheprovider", "-k", spec["select"]],
                             capture_output=True, text=True, timeout=600, cwd=root, env=env)
        ids = lambda word: sorted(l.split("::", 1)[1].split(" ")[0] for l in out.stdout.splitlines() if l.startswith(word + " ") and "::" in l)
        return out, ids("PASSED"), ids("FAILED")
    out, passed, failed = run("mut%d" % mutant)
    assert out.returncode == 1, (out.stdout[-1500:], out.stderr[-1500:])
    for want in spec["must_fail"]:     # every id in full: both launch sets where both must fail
        assert want in failed, (want, failed, passed)
    for want in spec["must_pass"]:
        assert want in passed and want not in failed, (want, failed, passed)
    assert "quad" in out.stdout   # the stage that differs: the quad list
    out_ok, passed_ok, failed_ok = run(None)
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
