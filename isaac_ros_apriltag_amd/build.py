"""Builds the native pieces of the package in-tree (the .so files travel to the GPU box with the repo).

  libapriltag_amd.so    HIP kernels + C ABI (hipcc, gfx950 only)         <- csrc/detector.hip
  libapriltag_amd.resources.txt   registers, spills, scratch, LDS and occupancy per kernel, as that compile reported them
  libapriltag_synth.so  deterministic frame renderer (host C)            <- csrc/synth_render.c
  libapriltag_node.so   ROS-free C++ mirror of the reference node shell  <- csrc/node_shell.cpp (if present)
  examples/multi_stream_host   C++ multi-GPU front end (RCCL broadcast)  <- examples/multi_stream_host.cpp
"""
import os
import re
import shutil
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
LIB_AMD = os.path.join(_HERE, "libapriltag_amd.so")
LIB_SYNTH = os.path.join(_HERE, "libapriltag_synth.so")
LIB_NODE = os.path.join(_HERE, "libapriltag_node.so")
# what the compiler reported per kernel of libapriltag_amd.so (registers, spills, private segment, LDS, occupancy): written by
# build_amd() from the remarks of the product compile itself, read by tests/test_kernel_scratch_cpu.py and tools/kernel_resources.py
RESOURCES_AMD = os.path.join(_HERE, "libapriltag_amd.resources.txt")
_REMARK = "-Rpass-analysis=kernel-resource-usage"   # a remark: does not change code generation


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _sources(*exts):
    inc = os.path.join(os.path.dirname(_HERE), "include")
    out = []
    for d in (_CSRC, inc):
        for f in sorted(os.listdir(d)):
            if f.endswith(exts):
                out.append(os.path.join(d, f))
    return out


def _demangle(names):
    for f in (os.path.join(os.path.dirname(_hipcc()), "..", "llvm", "bin", "llvm-cxxfilt"), shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if f and os.path.exists(f):
            out = subprocess.run([f] + list(names), capture_output=True, text=True).stdout.splitlines()
            if len(out) == len(names):
                return out
    return list(names)


def resource_remarks(stderr_text):
    """The kernel-resource-usage remarks of a hipcc run as text: per kernel one "Function Name: <demangled name without arguments>"
    line, then its "    <field>: <number>" lines as the compiler printed them (units dropped); and what else the compiler said."""
    kernels, rest, skip = [], [], 0
    for line in stderr_text.splitlines():
        if _REMARK in line:
            m = re.search(r"remark:\s+([A-Za-z ]+\w)(?: \[[^\]]*\])?: (\S+) \[" + _REMARK, line)
            if m and m.group(1) == "Function Name":
                kernels.append((m.group(2), []))
                skip = 2   # the source line and the caret under it
            elif m and kernels:
                kernels[-1][1].append("    %s: %s" % (m.group(1), m.group(2)))
        elif skip and not line.startswith("In file included"):
            skip -= 1
        elif not (line.startswith("In file included") or re.match(r"\d+ (warning|remark)s? generated", line.strip())):
            rest.append(line)
    names = _demangle([k for k, _ in kernels])
    text = "".join("Function Name: %s\n%s\n" % (n.split("(")[0].replace("void ", "", 1), "\n".join(f)) for n, (_, f) in zip(names, kernels))
    return text, "\n".join(rest)


def parse_resources(text):
    """{kernel name: {field: int}} of a file written by build_amd() (RESOURCES_AMD)."""
    rows, cur = {}, None
    for line in text.splitlines():
        if line.startswith("Function Name: "):
            cur = rows.setdefault(line[len("Function Name: "):].strip(), {})
        elif cur is not None and ": " in line:
            k, v = line.strip().rsplit(": ", 1)
            if v.isdigit():
                cur[k] = int(v)
    return rows


def build_amd(force=False):
    srcs = _sources(".hip", ".h")
    if force or _newer(LIB_AMD, srcs) or not os.path.exists(RESOURCES_AMD):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
               "-fno-fast-math", "-Wall", "-Wno-unused-value", "-Wno-unused-function", "-Wno-pass-failed", _REMARK,
               os.path.join(_CSRC, "detector.hip"), "-o", LIB_AMD]
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        text, rest = resource_remarks(r.stderr)
        if rest.strip():
            sys.stderr.write(rest + "\n")
        if r.returncode:
            raise subprocess.CalledProcessError(r.returncode, cmd)
        with open(RESOURCES_AMD, "w") as f:
            f.write(text)
    return LIB_AMD


def build_amd_variant(tag, defines):
    """Measurement builds for tools/ (e.g. -DAMDAT_FQ_PROFILE: per-phase cycle counters in the quad-fit kernel).
    The product library carries none of this; the variant is written next to it as libapriltag_amd_<tag>.so.
    An entry of `defines` that starts with "-" is passed to the compiler as it stands (e.g. "-mllvm", "-amdgpu-sched-strategy=max-ilp")."""
    out = os.path.join(_HERE, "libapriltag_amd_%s.so" % tag)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
           "-fno-fast-math", "-Wno-unused-value", "-Wno-unused-function", "-Wno-pass-failed"] + \
          [d if d.startswith("-") else "-D" + d for d in defines] + \
          [os.path.join(_CSRC, "detector.hip"), "-o", out]
    subprocess.check_call(cmd)
    return out


def build_synth(force=False):
    src = os.path.join(_CSRC, "synth_render.c")
    if force or _newer(LIB_SYNTH, [src] + _sources(".h")):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-std=gnu99", "-ffp-contract=off", "-shared", "-o", LIB_SYNTH,
                               src, "-lm"])
    return LIB_SYNTH


def build_node(force=False):
    src = os.path.join(_CSRC, "node_shell.cpp")
    if not os.path.exists(src):
        return None
    if force or _newer(LIB_NODE, [src] + _sources(".h", ".hpp")):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", LIB_NODE, src, "-ldl"])
    return LIB_NODE


HOST_BIN = os.path.join(os.path.dirname(_HERE), "examples", "multi_stream_host")


def build_host(force=False):
    """C++ multi-GPU front end (one handle per device, RCCL broadcast of the parameter block)."""
    src = os.path.join(os.path.dirname(_HERE), "examples", "multi_stream_host.cpp")
    if not os.path.exists(src):
        return None
    if force or _newer(HOST_BIN, [src, LIB_AMD] + _sources(".h")):
        subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(os.path.dirname(_HERE), "include"),
                               src, "-L" + _HERE, "-lapriltag_amd", "-lrccl", "-Wl,-rpath," + _HERE, "-o", HOST_BIN])
    return HOST_BIN


LIB_STRESS = os.path.join(_HERE, "libapriltag_amd_stress.so")


def build_stress(force=False):
    """Stress build for the GPU suite (tests/test_gpu_parity.py::test_long_staging_records...): a 64 x 16 tile's emission list
    is cut to 768 entries, so that on ordinary frames a good share of the boundary points takes the long-record path that the
    product build only enters above two emissions per pixel of a tile; and the cluster list starts at 1024 entries instead of
    65 536, so that the noisy 1080p frames (4 000 clusters) make it grow twice.  Never loaded by the product path."""
    if force or _newer(LIB_STRESS, [os.path.join(_CSRC, "detector.hip")] + _sources(".h")):
        build_amd_variant("stress", ["PT_ELIST=768", "AMDAT_LCAP_DIV=1", "AMDAT_CCAP0=1024u"])
    return LIB_STRESS


MUTANTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40,
           41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58)   # csrc/tools_hooks.h, AMDAT_MUTATE
MUTANT_JOBS = 16   # compilers build_mutants runs at a time


def lib_mutant(n):
    return os.path.join(_HERE, "libapriltag_amd_mut%d.so" % n)


def build_mutants(force=False):
    """Deliberately WRONG builds of the same sources (csrc/tools_hooks.h: -DAMDAT_MUTATE=1 the launch sequence without k_fit_small,
    2 one row constant off in k_cc_local<4>, 3 one sector too many in k_fit_prefilter<64>'s test, 4 k_quad_sigma's copy rule with the
    padded half width on the far edges, 5 no edge refinement when the quad_sigma filter runs at decimate > 1, 6 k_cluster_select with the
    handle's cluster-size cap for a smaller frame of a per-frame-sizes submission, 7 a quarter of the line-fit limit in the group test
    of k_fit_quads<256> and <1024>, 8 the last wave's totals twice in the chunk carry of the general moment sweep, 9 the rectification's
    fixed-point source position truncated instead of rounded, 10 every frame of a rectified submission with the first camera's model,
    11 the resize's source position without the half-pixel term, 12 every frame of a resized submission with the first target size,
    13 the general camera projection without its rectification rotation, 14 the rational_polynomial model without its denominator, 15 k_bundle_pose with the
    record corners in the order p[3 - k], 16 k_bundle_pose without the duplicate rule, 17 the pose refinement's second chain started
    unmirrored, 18 the pose refinement without t(R) after its last iteration, 19 the object points of a rigid bundle without the member's
    rotation, 20 the means of the rigid bundle's iteration divided by 4 instead of 4 * ntags, 21 the edge refinement counting steps
    outside the image, 22 the code scan keeping the higher index at equal distance, 23 the overlap test of k_reconcile without containment,
    24 k_reconcile's order with margins ascending, 25 the pose covariance without the skew term in J_u, 26 the second quad of
    k_pose_refine<true> at chain 0's pose, 27 a rigid bundle's covariance with centred object points, 28 the corner undistortion without its rectification rotation, 29 the
    pose launches on the raw records with the corner undistortion on, 30 every frame of an undistorted submission with the first
    camera's model, 31 the one-pass threshold's low-contrast rule with <=, 32 k_threshold_leftover with >= against the threshold,
    33 cc_row_requests' up-link skip without the left-source guard, 34 k_cc_resolve with > against min_component_size, 35 k_points'
    general form with every left neighbour a source, 36 k_cluster_select with > against min_cluster_points, 37 k_quad_finish's area
    limit as 1.0 * w * w, 38 k_quad_finish without the lower angle test, 39 k_quad_finish without the winding term,
    40 fit_border_unwanted without its normal_border statement, 41 .. 44 the cut to max_nmaxima corners keeping nine in k_fit_small and
    in k_fit_quads with up to 64, up to 64 * FQ_SEL_REGS and more maxima, 45 the corner search without its dot test, 46 the rig pose's translation
    statement without the ray origin, 47 the rig pose's ray direction with Rc in place of its transpose, 48 k_bundle_rig's observation
    slots cut at 63, 49 the raw formats' reflect rule as a clamp at the right and bottom edge, 50 the horizontal and vertical averages
    exchanged at the green sites of blue rows, 51 the 16-bit sample with & 255 in place of the saturation, 52 the 16-bit Bayer instance
    without the x phase, 53 the tag table's binary search ending one entry early, 54 the tag table's wildcard consulted before the exact
    key, 55 k_pose_refine with the handle's tag_size for every record, 56 the code scan keeping a lane's later code at equal distance,
    57 the quarter turn's ballot without lane 63, 58 the border samples from index 64 on stored as invalid),
    shipped like the stress build so that the GPU suite itself shows, under the driver's eyes, that its stage tests FAIL on each of them
    (tests/test_gpu_parity.py::test_the_suite_fails_on_wrong_builds, tests/test_per_frame_sizes_gpu.py for 6,
    tests/test_fit_classes_gpu.py for 7 and 8, tests/test_rectify_submission_gpu.py for 9 and 10,
    tests/test_resize_submission_gpu.py for 11 and 12, tests/test_camera_models_gpu.py for 13 and 14, tests/test_bundles_gpu.py for 15 and 16,
    tests/test_pose_refine_gpu.py for 17 and 18, tests/test_rigid_bundles_gpu.py for 19 and 20, tests/test_decode_stage_gpu.py for
    21 .. 24, tests/test_pose_covariance_gpu.py for 25 .. 27, tests/test_corner_undistortion_gpu.py for 28 .. 30,
    tests/test_integer_stages_gpu.py for 31 .. 36, tests/test_fit_rules_gpu.py for 37 .. 45,
    tests/test_rig_bundles_gpu.py for 46 .. 48, tests/test_raw_formats_gpu.py for 49 .. 52, tests/test_tag_table_gpu.py for 53 .. 55,
    tests/test_decode_families_gpu.py for 56 .. 58).
    Never loaded by the product path.
    At most MUTANT_JOBS compilers run at a time."""
    from concurrent.futures import ThreadPoolExecutor
    err = []

    def _one(n):
        try:
            if force or _newer(lib_mutant(n), [os.path.join(_CSRC, "detector.hip")] + _sources(".h")):
                build_amd_variant("mut%d" % n, ["AMDAT_MUTATE=%d" % n])
        except (subprocess.CalledProcessError, OSError) as e:
            err.append(e)
    with ThreadPoolExecutor(max_workers=MUTANT_JOBS) as pool:
        list(pool.map(_one, MUTANTS))
    if err:
        raise err[0]
    return [lib_mutant(n) for n in MUTANTS]


def build_all(force=False):
    import threading
    build_synth(force)
    err = []

    def _stress():
        try:
            build_stress(force)
        except (subprocess.CalledProcessError, OSError) as e:   # only its test needs it
            err.append(e)

    def _mutants():
        try:
            build_mutants(force)
        except (subprocess.CalledProcessError, OSError) as e:   # only their test needs them
            err.append(e)
    t = threading.Thread(target=_stress)
    t.start()                      # (next to the product library: hipcc runs of the same translation unit)
    build_amd(force)
    t.join()
    tm = threading.Thread(target=_mutants)
    tm.start()
    tm.join()
    if err:
        import sys
        sys.stderr.write("isaac_ros_apriltag_amd.build: stress / mutant variants not built (%s); only their tests need them\n" % (err[0],))
    build_node(force)
    try:   # the multi-GPU example links RCCL; a machine without it still gets the product libraries
        build_host(force)
    except (subprocess.CalledProcessError, OSError) as e:
        import sys
        sys.stderr.write("isaac_ros_apriltag_amd.build: examples/multi_stream_host not built (%s); only its test needs it\n" % (e,))


if __name__ == "__main__":
    build_all(force=True)
    print("built", LIB_AMD, LIB_SYNTH)
