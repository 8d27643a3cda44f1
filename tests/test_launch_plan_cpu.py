"""Host checks of the launch schedule (isaac_ros_apriltag_amd/csrc/launch_plan.h): the size classes of the quad fit, their work
lists, and what one submission launches -- launch set, kernel instances, grids, and the order and streams of the fit's classes.
No result depends on any of it (the GPU parity suite cannot see a change here), only the speed does: the expected plans below are
the schedule as measured into place, written out literally."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

AUTO, LATENCY, THROUGHPUT = 0, 1, 2       # AMDAT_PATH_*
EMPTY, SMALL, QUADS = 0, 1, 2             # FqKernel


def handle(W, H):
    """max_cluster_points and split_moments of a W x H working image (amdCreateAprilTagsDetectorEx)."""
    mcp = 3 * (2 * W + 2 * H)
    return mcp, int(W <= 2048 and H <= 2048 and mcp < 32768)


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(HERE, "aux_c", "launch_plan_driver.cpp"), "-o", exe])

    def run(*words):
        out = subprocess.run([exe], input=" ".join(map(str, words)) + "\n", capture_output=True, text=True, check=True).stdout
        return out.strip()
    return run


def plan(drv, W, H, B, n, hcap, path=AUTO, cus=256, prefilter=1):
    mcp, split = handle(W, H)
    head, steps = drv("plan", mcp, split, cus, B, n, W, H, hcap, path, prefilter).split("|")
    keys = ("latency", "cc_waves", "border_per_wave", "cc_root_grid", "select_chunks", "select_grid", "decode_grid")
    return dict(zip(keys, map(int, head.split()))), steps.split()


# (B, n): launch set, k_cc_local waves, k_cc_border per wave, root grid, select chunks, select grid, decode grid | fit steps
# F: fork; P<threads>:grid:stream; C<class>[* compact list]:grid:pop:stream; stream s: the submission stream, 0 .. 2 side streams
HD = {
    (1, 1): "1 16 0 507 1 64 256 | F P1024:256:s C5*:64:1:s C6*:16:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2",
    (8, 1): "1 16 0 507 1 64 256 | F P1024:256:s C5*:512:1:s C6*:128:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2",
    (8, 4): "1 16 0 507 1 64 256 | F P1024:512:s C5*:512:1:s C6*:128:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2",
    (8, 5): "1 4 0 507 1 64 256 | F P1024:512:s C5*:512:1:s C6*:128:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2",
    (8, 8): "1 4 0 507 1 64 256 | F P1024:512:s C5*:512:1:s C6*:128:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2",
    (256, 1): "1 16 0 507 1 64 256 | F P1024:256:s C5*:512:1:s C6*:256:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2",
    (256, 4): "1 16 0 507 1 64 256 | F P1024:512:s C5*:512:1:s C6*:256:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2",
    (256, 5): "1 4 0 507 1 64 256 | F P1024:512:s C5*:512:1:s C6*:256:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2",
    (256, 8): "1 4 0 507 1 64 256 | F P1024:512:s C5*:512:1:s C6*:256:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2",
    (256, 256): "0 4 1 507 4 16 96 | P64:8192:s C5*:512:1:s C6*:256:1:s F C4*:1024:1:s C3:2048:2:0 C2:4096:4:1 C0:4096:4:2",
}


def expect(line):
    head, steps = line.split("|")
    keys = ("latency", "cc_waves", "border_per_wave", "cc_root_grid", "select_chunks", "select_grid", "decode_grid")
    return dict(zip(keys, map(int, head.split()))), steps.split()


@pytest.mark.parametrize("B,n", sorted(HD))
def test_1080p_plans(drv, B, n):
    # (from 5 frames on the CC limit -- 8 Mi px -- and the launch-set limit -- 16 Mi px -- disagree: latency set, k_cc_local<4>)
    assert plan(drv, 1920, 1080, B, n, 65536) == expect(HD[(B, n)])


def test_throughput_anchor(drv):
    """A 256-frame 1080p submission: the prefilter, then the two largest classes alone on the empty chip, then the fork."""
    p, steps = plan(drv, 1920, 1080, 256, 256, 65536)
    assert (p["latency"], p["cc_waves"], p["border_per_wave"], p["cc_root_grid"]) == (0, 4, 1, 507)
    assert (p["select_chunks"], p["select_grid"], p["decode_grid"]) == (4, 16, 96)
    assert steps[:3] == ["P64:8192:s", "C5*:512:1:s", "C6*:256:1:s"] and steps[3] == "F"
    assert steps[4:] == ["C4*:1024:1:s", "C3:2048:2:0", "C2:4096:4:1", "C0:4096:4:2"]


def test_latency_anchor(drv):
    """A one-frame 1080p submission: the fork first, so that the side streams' classes do not wait for the prefilter."""
    p, steps = plan(drv, 1920, 1080, 1, 1, 65536)
    assert (p["latency"], p["cc_waves"], p["border_per_wave"]) == (1, 16, 0)
    assert (p["select_chunks"], p["select_grid"], p["decode_grid"]) == (1, 64, 256)
    assert steps == ["F", "P1024:256:s", "C5*:64:1:s", "C6*:16:1:s", "C4:256:1:0", "C3:512:1:1", "C2:2048:1:2"]
    assert not any(s.startswith("C0") for s in steps)   # no k_fit_small on the latency set


def test_pinned_paths_override_the_size(drv):
    # the latency set for 256 frames keeps their own counts only where the set does not pin them: eight frames' chunks and pops
    assert plan(drv, 1920, 1080, 256, 256, 65536, path=LATENCY) == expect(
        "1 16 0 507 1 64 96 | F P1024:512:s C5*:512:1:s C6*:256:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2")
    # and the throughput set for one frame takes 64 frames' chunks and pops
    assert plan(drv, 1920, 1080, 256, 1, 65536, path=THROUGHPUT) == expect(
        "0 4 1 507 4 16 256 | P64:256:s C5*:512:1:s C6*:256:1:s F C4*:1024:1:s C3:2048:2:0 C2:4096:4:1 C0:4096:4:2")


def test_small_image_without_prefilter(drv):
    """160 x 120: no cluster above 2048 points, no prefilter.  From 3496 frames on (64 Mi px) the large classes would run first;
    they are empty at this size, so only the side streams of the small classes differ."""
    assert plan(drv, 160, 120, 1, 1, 4096) == expect("1 16 0 5 1 4 256 | F C3:512:1:2 C2:2048:1:0")
    assert plan(drv, 160, 120, 3495, 3495, 4096)[1] == ["F", "C3:2048:2:2", "C2:4096:4:0", "C0:4096:4:2"]
    assert plan(drv, 160, 120, 3496, 3496, 4096) == expect("0 4 1 5 4 1 96 | F C0:4096:4:0 C2:4096:4:1 C3:2048:2:2")


def test_tiny_image_still_launches_the_one_wave_class(drv):
    """A 9 x 8 working image (the fuzzer's, round 5): no cluster can exceed k_fit_small's bound, but the latency set buckets its
    clusters into the one-wave class, which must launch."""
    assert plan(drv, 9, 8, 1, 1, 4096) == expect("1 16 0 1 1 4 256 | F C2:2048:1:0")
    assert plan(drv, 9, 8, 1, 1, 4096, path=THROUGHPUT)[1] == ["F", "C0:4096:4:2"]


def test_large_image_has_no_k_fit_small(drv):
    """Working images above 2048: no two-double moments, so no k_fit_small class; the one-wave class takes everything up to 768."""
    assert plan(drv, 4096, 2160, 1, 1, 524288) == expect(
        "1 4 0 1024 1 512 256 | F P1024:256:s C5*:64:1:s C6*:16:1:s C4:256:1:0 C3:512:1:1 C2:2048:1:2")
    assert plan(drv, 4096, 2160, 8, 8, 524288, path=THROUGHPUT) == expect(
        "0 4 1 1024 4 128 256 | P64:2048:s C5*:512:1:s C6*:128:1:s F C4*:1024:1:s C3:2048:2:0 C2:4096:4:1")


def test_other_cu_count(drv):
    assert plan(drv, 1920, 1080, 256, 256, 65536, cus=304) == expect(
        "0 4 1 507 4 16 96 | P64:9728:s C5*:608:1:s C6*:304:1:s F C4*:1216:1:s C3:2432:2:0 C2:4864:4:1 C0:4864:4:2")
    assert plan(drv, 1920, 1080, 1, 1, 65536, cus=304) == expect(
        "1 16 0 507 1 64 256 | F P1024:256:s C5*:64:1:s C6*:16:1:s C4:256:1:0 C3:608:1:1 C2:2432:1:2")


def test_without_the_prefilter(drv):
    """Builds without the prefilter (-DAMDAT_FQ_NO_PREFILTER): the longest chains side by side, or the large classes first from
    64 Mi px on."""
    assert plan(drv, 1920, 1080, 1, 1, 65536, prefilter=0)[1] == [
        "F", "C6:16:1:s", "C5:64:1:0", "C4:256:1:1", "C3:512:1:2", "C2:2048:1:0"]
    assert plan(drv, 1920, 1080, 256, 256, 65536, prefilter=0)[1] == [
        "C5:512:1:s", "C6:256:1:s", "F", "C0:4096:4:0", "C2:4096:4:1", "C3:2048:2:2", "C4:1024:1:0"]


def test_class_table(drv):
    rows = lambda out: [tuple(map(int, r.split())) for r in out.split("|")[0].split(";") if r.strip()]
    # nt, sort_cap, (lo, hi], grid, slot_cap, pop, kernel
    out = drv("classes", *handle(1920, 1080), 256, 256)
    assert rows(out) == [(64, 0, 0, 128, 4096, 128, 4, SMALL), (64, 0, 128, 128, 0, 0, 0, EMPTY),
                         (64, 768, 128, 768, 4096, 768, 4, QUADS), (128, 2048, 768, 2048, 2048, 2048, 2, QUADS),
                         (256, 4096, 2048, 4096, 1024, 4096, 1, QUADS), (512, 8192, 4096, 8192, 512, 8192, 1, QUADS),
                         (1024, 18048, 8192, 0x7FFFFFFF, 256, 18000, 1, QUADS)]   # (the key array holds the largest cluster)
    assert int(out.split("|")[1]) == 4                                             # the prefilter's first class
    out = drv("classes", *handle(4096, 2160), 256, 1)                              # no k_fit_small; grids follow one frame
    assert rows(out)[0] == (64, 0, 0, 0, 4096, 0, 4, SMALL) and rows(out)[2] == (64, 768, 0, 768, 4096, 768, 4, QUADS)
    assert [r[4] for r in rows(out)[3:]] == [1024, 256, 64, 16] and rows(out)[6][5] == 37536
    assert rows(out)[6][1] == 16384
    assert rows(drv("classes", *handle(40, 30), 256, 1))[6][5] == 8193


def test_work_layouts(drv):
    """1080p, 256 frames, one point per pixel and 65 536 clusters per frame: every list holds what its smallest clusters allow, on
    either set (the latency set buckets everything from 24 points on into the one-wave class)."""
    out = drv("layouts", *handle(1920, 1080), 256, 256, 2073600, 65536).split("|")
    assert int(out[0]) == 0 and int(out[3]) == 34699024
    lists = lambda s: [tuple(map(int, r.split())) for r in s.split(";") if r.strip()]
    assert lists(out[1]) == [(23, 128, 0, 16777216), (128, 128, 16777216, 16), (128, 768, 16777232, 16777216),
                             (768, 2048, 33554448, 690432), (2048, 4096, 34244880, 259328), (4096, 8192, 34504208, 129792),
                             (8192, 0x7FFFFFFF, 34634000, 65024)]
    assert lists(out[2]) == [(23, 0, 0, 16777216), (23, 0, 16777216, 16), (23, 768, 16777232, 16777216)] + lists(out[1])[3:]


def test_batch_too_large(drv):
    assert int(drv("layouts", *handle(1920, 1080), 256, 16384, 2073600, 65536).split("|")[0]) == 0
    assert int(drv("layouts", *handle(1920, 1080), 256, 32768, 2073600, 65536).split("|")[0]) == 6   # AMDAT_BATCH_TOO_LARGE
