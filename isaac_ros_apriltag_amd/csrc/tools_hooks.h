// tools_hooks.h -- every measurement hook of the kernels, in one place.  The PRODUCT build defines none of the AMDAT_*
// switches below, so every macro here expands to nothing and the kernel sources carry no conditional code of their own.
// Tools builds (isaac_ros_apriltag_amd.build.build_amd_variant, tools/*.sh) switch single hooks on:
//   -DAMDAT_FQ_PROFILE      shader-cycle counters per phase of k_fit_quads / k_fit_prefilter / k_points (prof[] slots)
//   -DAMDAT_FQ_TIMELINE     wall-clock log of every cluster k_fit_quads processes (tools/fit_timeline_one.py)
//   -DAMDAT_FQ_STOP=n       k_fit_quads drops every cluster after phase n   (instruction counts per phase, tools/fq_phase_insts.sh)
//   -DAMDAT_PT_STOP=n       k_points returns after phase n                  (tools/pt_phase_insts.sh)
//   -DAMDAT_CC_STOP=n       k_cc_local returns after phase n
//   -DAMDAT_FQ_SKIP=mask    the launch sequence leaves out k_fit_quads classes (bits 0..4) or the prefilter (bit 5)
//   -DAMDAT_FQ_NO_*         one of the quad fit's sound early exits compiled out (see below)
//   -DAMDAT_MUTATE=n        a deliberately WRONG build for tools/mutation_check.sh, which shows that the GPU suite fails on it:
//                           1 = the launch sequence leaves out k_fit_small (the throughput set's small-cluster fit);
//                           2 = k_cc_local<4> writes the wrong row as its tile's last perimeter row (one row constant off in the 4-wave instance only)
//                           3 = k_fit_prefilter<64>'s 64-sector test counts one sector too many at either end of every forward arc
//                               (the cut sectors themselves, which hold the corners): it then "proves" real quads above 2048 points
//                               impossible and drops them
//                           4 = k_quad_sigma's copy rule takes the instance's padded half width KH for the tap half width h on the right
//                               and bottom edges: wrong values in the last KH - h filtered columns / rows, for h < KH only (h = 3, 5, 6, 7)
//                           5 = with the quad_sigma filter on at decimate > 1 the decode launch runs as if refine_edges were 0
//                           6 = k_cluster_select takes the cluster-size cap from the handle instead of the frame: a smaller frame of a
//                               per-frame-sizes submission keeps clusters above its own cap (the scratch slots are sized by the handle's cap)
//                           7 = the group test after the first walk of the two-double sweep (fq_feasible, k_fit_quads<256, true> and
//                               <1024, true> only) is handed a quarter of max_line_fit_mse: it then "proves" quads impossible whose sides
//                               fit a line at a mean square error between a quarter of the limit and the limit, and drops them
//                           8 = the general sweep of k_fit_quads<NT, false>, NT >= 128 (working images above 2048 pixels a side): the last
//                               wave's totals enter the running carry from chunk to chunk twice, so every prefix behind a chunk's end is
//                               too large by them.  (Twice, not once too few or with the wrong sign: the prefixes stay the increasing,
//                               positive moments of a point set -- the cluster with some points counted double -- so no window has a
//                               weight of zero or below, nothing downstream meets a NaN or an infinity it does not meet in the product
//                               build, and the wrong build can only give wrong quads.)
//                           9 = the rectification statement (kernels_frontend.h: rect_taps) truncates the fixed-point source position,
//                               (int)(u * 32.0) without the + 0.5: taps and weights one 1/32 step low wherever the fraction is a half or more
//                           10 = amdAprilTagsSetRectification: every frame of a submission takes cams[0] instead of cams[i % ncams]
//                           11 = the resize statement (kernels_frontend.h: resize_pos) without the half-pixel term: the source
//                               position (2i * sn * 1024) / dn instead of ((2i + 1) * sn * 1024) / dn - 1024 (indices clamped as before)
//                           12 = amdAprilTagsSetResize: every frame of a submission takes sizes[0] instead of sizes[i % nsizes]
//                           13 = the general projection (camera_models.h) takes the identity for the transpose of the rectification
//                               rotation: a camera with R is rectified as if it had none
//                           14 = the general projection takes 1 for the denominator of rational_polynomial's radial factor: k4 .. k6 are ignored
//                           15 = k_bundle_pose pairs board corner k of a member with the record's corner p[3 - k]: every solved bundle
//                               gets a wrong pose (a frame without tags is unaffected)
//                           16 = k_bundle_pose without the duplicate rule: the records of a (family, id) seen twice in a frame are used
//                           17 = chain 1 of the pose refinement (pose_refine.h) starts at the homography pose itself, unmirrored: the
//                               alternative of every refined record is the chosen pose again
//                           18 = the pose refinement does not recompute t after the last iteration: every refined record carries the
//                               last rotation with the translation of the one before
//                           19 = the object points of a rigid bundle (rigid_layout.h) ignore the member's R: every member is taken
//                               as axis-parallel to the bundle frame
//                           20 = the means of the rigid bundle's iteration (rigid_pose.h) are divided by 4, section 7e's per-tag
//                               count, instead of 4 * ntags: wrong wherever two or more tags are used
//                           21 = the edge refinement (k_decode_wave) counts a step of the normal search with a read outside the image, with
//                               pixel 0's value in that read's place: wrong only where a tag's side lies within a few pixels of the frame edge
//                           22 = the code scan's wave reduction (k_decode_wave) keeps the HIGHER index at equal distance: wrong only where
//                               two codes of a family are equally near the word read (tag16h5 at max_hamming 3)
//                           23 = quads_overlap_dev (k_reconcile) without its two containment tests: a duplicate strictly inside another
//                               record of its id survives
//                           24 = det_before_dev (k_reconcile) compares decision margins ascending
//                           25 = the pose covariance (pose_covariance.h) leaves the skew term b out of J_u: wrong only under a camera
//                               with skew
//                           26 = the second quad of k_pose_refine<true> evaluates the covariance at chain 0's pose: cov_alt equals cov
//                           27 = the covariance of a rigid bundle takes P - mean P for the object point P
//                           28 = the corner undistortion (undistort.h) takes the identity for the rectification rotation R
//                           29 = with amdAprilTagsSetCornerUndistortion on, the bundle and refinement launches still read the raw
//                               records (d_dets, not d_dets_u: two live buffers of one size)
//                           30 = amdAprilTagsSetCornerUndistortion: every frame of a submission takes cams[0] instead of cams[i % ncams]
//                           31 = the low-contrast rule of the one-pass k_threshold (tile size 4) as mx - mn <= min_white_black_diff:
//                               wrong only in a tile whose dilated range is exactly min_white_black_diff (5)
//                           32 = k_threshold_leftover compares v >= thresh: wrong only where a pixel right of / below the last full
//                               tile equals its nearest tile's threshold
//                           33 = cc_row_requests (k_cc_border) skips the up link without asking whether the left neighbour is a link
//                               source: wrong only at x = 1 on a tile-top row, where column 0 carries no link
//                           34 = k_cc_resolve sets the size bit for a count > min_component_size: wrong only for a component that
//                               reaches exactly min_component_size (25) pixels across tiles
//                           35 = the general form of k_points takes every left neighbour for an emission source: wrong only at x = 1
//                           36 = k_cluster_select keeps a pair for a count > min_cluster_points: wrong only for a cluster of exactly
//                               min_cluster_points (24) points
//                           37 = k_quad_finish's area limit as 1.0 * w * w: wrong only for a quad whose Heron area lies in
//                               [0.95 w^2, w^2), w = min_tag_width
//                           38 = k_quad_finish without cos_dtheta < -cos_critical_rad: a quad with a corner sharper than 10 degrees is kept
//                           39 = k_quad_finish without the winding term: a quad whose corners turn the wrong way (a dart) is kept
//                           40 = fit_border_unwanted without its normal_border statement: a handle whose families all have a reversed
//                               border keeps the quads of normal borders
//                           41 .. 44 = the cut to max_nmaxima corners takes its threshold from rank max_nmaxima - 1 and so keeps nine:
//                               41 in k_fit_small, 42 in k_fit_quads with up to 64 maxima, 43 with up to 64 * FQ_SEL_REGS, 44 above;
//                               wrong only where a corner of the chosen set is the tenth largest maximum
//                           45 = fq_corner_search without its dot test: a corner choice whose first two sides are nearly parallel is
//                               admitted
//                           46 = the translation statement of the rig pose (rig_pose.h) leaves the ray origin out: wrong wherever a
//                               camera of the rig is not at the rig's origin
//                           47 = the ray direction of the rig pose takes Rc in place of its transpose: wrong wherever a camera of the
//                               rig is turned against the rig frame
//                           48 = k_bundle_rig cuts the observation slots at 63: wrong only where a (group, bundle) has 64 or more
//                               used observations
//                           49 = the raw formats' reflect rule (raw_formats.h) clamps at the right and bottom edge, n - 1 in place of
//                               2 (n - 1) - i (an index inside the frame): wrong only in the last column and row of a Bayer frame
//                           50 = the green sites of blue rows take the horizontal average for red and the vertical one for blue
//                           51 = the sample of a 16-bit encoding is (s >> shift) & 255: wrong only where s >= 256 << shift
//                           52 = the 16-bit Bayer instance ignores the x phase: grbg16 and bggr16 are demosaiced as rggb16 and gbrg16
//                           53 = the tag table's binary search (tag_table.h: tt_find) ends one entry early: the last key is never found
//                           54 = the tag table's lookup consults the family's wildcard before the exact key: wrong only where an
//                               exact entry sits beside a wildcard of its family
//                           55 = k_pose_refine keeps the handle's tag_size: wrong only in refined poses and covariances of tags whose
//                               table size differs from it, never in a detection record
//                           56 = the code scan (k_decode_wave) keeps a lane's LATER code at equal distance (hd <= best over c += 64): wrong
//                               only where two equally near codes of a family have indices congruent mod 64
//                           57 = the quarter turn's ballot (k_decode_wave) leaves lane 63 out: wrong only for a 64-bit family read turned
//                           58 = the border samples of the gray models (k_decode_wave) are stored as invalid from index 64 on, the sample
//                               loop's second trip: wrong only for a family with width_at_border 9 or 10
//                           (4 .. 58 change values only: no address outside the frame, index bound or launch size; 43 and 44 run their
//                           removal loop one round less; 53 reads one entry less)
//                           the GPU suite ships them all (build.py: build_mutants) and asserts that its stage tests FAIL on each
//                           (tests/test_gpu_parity.py::test_the_suite_fails_on_wrong_builds for 1 .. 5,
//                           tests/test_per_frame_sizes_gpu.py::test_cluster_cap_fails_on_the_wrong_build for 6,
//                           tests/test_fit_classes_gpu.py::test_fit_class_tests_fail_on_the_wrong_builds for 7 and 8,
//                           tests/test_rectify_submission_gpu.py::test_the_rectify_tests_fail_on_the_wrong_builds for 9 and 10,
//                           tests/test_resize_submission_gpu.py::test_the_resize_tests_fail_on_the_wrong_builds for 11 and 12,
//                           tests/test_camera_models_gpu.py::test_the_camera_model_tests_fail_on_the_wrong_builds for 13 and 14,
//                           tests/test_bundles_gpu.py::test_the_bundle_tests_fail_on_the_wrong_builds for 15 and 16,
//                           tests/test_pose_refine_gpu.py::test_the_pose_refinement_tests_fail_on_the_wrong_builds for 17 and 18,
//                           tests/test_rigid_bundles_gpu.py::test_the_rigid_bundle_tests_fail_on_the_wrong_builds for 19 and 20,
//                           tests/test_decode_stage_gpu.py::test_the_decode_stage_tests_fail_on_the_wrong_builds for 21 .. 24,
//                           tests/test_pose_covariance_gpu.py::test_the_pose_covariance_tests_fail_on_the_wrong_builds for 25 .. 27,
//                           tests/test_corner_undistortion_gpu.py::test_the_undistortion_tests_fail_on_the_wrong_builds for 28 .. 30,
//                           tests/test_integer_stages_gpu.py::test_integer_stage_tests_fail_on_the_wrong_builds for 31 .. 36,
//                           tests/test_fit_rules_gpu.py::test_the_fit_rule_tests_fail_on_the_wrong_builds for 37 .. 45,
//                           tests/test_rig_bundles_gpu.py::test_the_rig_tests_fail_on_the_wrong_builds for 46 .. 48,
//                           tests/test_raw_formats_gpu.py::test_the_raw_format_tests_fail_on_the_wrong_builds for 49 .. 52,
//                           tests/test_tag_table_gpu.py::test_the_tag_table_tests_fail_on_the_wrong_builds for 53 .. 55,
//                           tests/test_decode_families_gpu.py::test_the_family_tests_fail_on_the_wrong_builds for 56 .. 58)
// The stop builds key on P.max_nmaxima == 10 (always true) so that the compiler cannot fold the early exit at compile time
// into dead-code elimination of the phases before it.
#pragma once

// -DAMDAT_ASM_MARKS: phase markers as assembler comments (static instruction counts per phase from hipcc -S)
#ifdef AMDAT_ASM_MARKS
#define AT_MARK(name) asm volatile("; ==MARK " name);
#else
#define AT_MARK(name)
#endif

// ---- k_cc_local ---------------------------------------------------------------------------------------------------------
#ifdef AMDAT_CC_STOP
#define CC_STOP_AT(n) if (AMDAT_CC_STOP == (n) && P.max_nmaxima == 10) return;
#else
#define CC_STOP_AT(n)
#endif

#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 2
#define CC_LAST_ROW_OFFSET(NW) ((NW) == 4 ? 2 : 1)
#else
#define CC_LAST_ROW_OFFSET(NW) 1
#endif

// ---- the integer stages: the low-contrast rule of the one-pass k_threshold; "white" in k_threshold_leftover; whether the up link's
// ---- skip rule of cc_row_requests may rely on the left neighbour; "large enough" in k_cc_resolve; whether the left neighbour of a
// ---- pixel of k_points' general form is an emission source; "enough points" in k_cluster_select ------------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 31
#define TH_LOW_CONTRAST(range, min_diff) ((range) <= (min_diff))
#else
#define TH_LOW_CONTRAST(range, min_diff) ((range) < (min_diff))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 32
#define TH_STRIP_WHITE(v, thresh) ((v) >= (thresh))
#else
#define TH_STRIP_WHITE(v, thresh) ((v) > (thresh))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 33
#define CC_ROW_UP_LEFT_SRC(left_src) ((void)(left_src), true)
#else
#define CC_ROW_UP_LEFT_SRC(left_src) (left_src)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 34
#define CC_RESOLVE_LARGE(size, min_size) ((size) > (min_size))
#else
#define CC_RESOLVE_LARGE(size, min_size) ((size) >= (min_size))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 35
#define PT_LEFT_IS_SOURCE(is_source) ((void)(is_source), true)
#else
#define PT_LEFT_IS_SOURCE(is_source) (is_source)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 36
#define SEL_ENOUGH_POINTS(count, min_points) ((count) > (min_points))
#else
#define SEL_ENOUGH_POINTS(count, min_points) ((count) >= (min_points))
#endif

// ---- the quad fit's rules: k_quad_finish's area limit (w: min_tag_width), its lower angle test and its winding term (a: dx1 * dy2,
// ---- b: dy1 * dx2); the normal_border statement of fit_border_unwanted; and the rank whose value is the threshold of the cut to
// ---- max_nmaxima corners (n), per site: 0 k_fit_small, 1 k_fit_quads up to 64 maxima, 2 up to 64 * FQ_SEL_REGS, 3 above ----------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 37
#define QF_AREA_LIMIT(w) (1.0 * (w) * (w))
#else
#define QF_AREA_LIMIT(w) (0.95 * (w) * (w))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 38
#define QF_COS_BELOW(c, crit) ((void)(c), (void)(crit), false)
#else
#define QF_COS_BELOW(c, crit) ((c) < -(crit))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 39
#define QF_WINDING_WRONG(a, b) ((void)(a), (void)(b), false)
#else
#define QF_WINDING_WRONG(a, b) ((a) < (b))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 40
#define FIT_NORMAL_UNWANTED(P, reversed) ((void)(reversed), false)
#else
#define FIT_NORMAL_UNWANTED(P, reversed) (!(P).normal_border && !(reversed))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE >= 41 && AMDAT_MUTATE <= 44
#define FIT_CUT_RANK(site, n) ((site) == AMDAT_MUTATE - 41 ? (n) - 1 : (n))
#else
#define FIT_CUT_RANK(site, n) (n)
#endif
// what fq_corner_search's dot test compares with cos_critical_rad (d: the dot product of the first two sides' normals)
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 45
#define FQ_DOT_SIZE(d) ((void)(d), 0.0)
#else
#define FQ_DOT_SIZE(d) fabs(d)
#endif

// ---- k_quad_sigma: the half width of the copy rule on the far (right / bottom) edge of a pass --------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 4
#define QS_FAR_EDGE_H(KH, h) (KH)
#else
#define QS_FAR_EDGE_H(KH, h) (h)
#endif

// ---- rectification: the source position in 1/32 pixel, and the camera model of batch slot i ------------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 9
#define RECT_FIXED(u) ((int)((u) * 32.0))
#else
#define RECT_FIXED(u) ((int)((u) * 32.0 + 0.5))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 10
#define RECT_MODEL_OF_SLOT(i, ncams) ((void)(i), (void)(ncams), 0u)
#else
#define RECT_MODEL_OF_SLOT(i, ncams) ((i) % (ncams))
#endif

// ---- the general projection: entry j of the transposed rectification rotation, and the rational model's denominator -------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 13
#define CAM_RI(Ri, j) ((void)(Ri), ((j) % 4 == 0 ? 1.0 : 0.0))
#else
#define CAM_RI(Ri, j) ((Ri)[j])
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 14
#define CAM_RATIONAL_DEN(den) ((void)(den), 1.0)
#else
#define CAM_RATIONAL_DEN(den) (den)
#endif

// ---- corner undistortion: entry j of the rectification rotation (undistort.h), the records the pose launches read with the mode on
// ---- (raw: d_dets, und: d_dets_u), and the camera model of batch slot i -----------------------------------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 28
#define UD_R(R, j) ((void)(R), ((j) % 4 == 0 ? 1.0 : 0.0))
#else
#define UD_R(R, j) ((R)[j])
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 29
#define UD_POSE_RECORDS(raw, und) ((void)(und), (raw))
#else
#define UD_POSE_RECORDS(raw, und) ((void)(raw), (und))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 30
#define UD_MODEL_OF_SLOT(i, ncams) ((void)(i), (void)(ncams), 0u)
#else
#define UD_MODEL_OF_SLOT(i, ncams) ((i) % (ncams))
#endif

// ---- resize: the source position in 1/2048 pixel of destination index i, and the target size of batch slot i -------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 11
#define RESIZE_FIXED(i, sn, dn) (((long long)(2 * (i)) * (sn) * 1024) / (dn))
#else
#define RESIZE_FIXED(i, sn, dn) (((long long)(2 * (i) + 1) * (sn) * 1024) / (dn) - 1024)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 12
#define RESIZE_SIZE_OF_SLOT(i, nsizes) ((void)(i), (void)(nsizes), 0u)
#else
#define RESIZE_SIZE_OF_SLOT(i, nsizes) ((i) % (nsizes))
#endif

// ---- k_bundle_pose: the record corner that is board corner k, and the duplicate rule ---------------------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 15
#define BUNDLE_PIXEL_CORNER(k) (3 - (k))
#else
#define BUNDLE_PIXEL_CORNER(k) (k)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 16
#define BUNDLE_DUPLICATE(dup) ((void)(dup), false)
#else
#define BUNDLE_DUPLICATE(dup) (dup)
#endif

// ---- pose_refine.h: the start of chain 1, and whether t(R) follows step `it` of `iterations` -------------------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 17
#define POSE_CHAIN1_START(mirrored, unmirrored) ((void)(mirrored), (unmirrored))
#else
#define POSE_CHAIN1_START(mirrored, unmirrored) ((void)(unmirrored), (mirrored))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 18
#define POSE_T_FOLLOWS_STEP(it, iterations) ((it) + 1u < (iterations))
#else
#define POSE_T_FOLLOWS_STEP(it, iterations) ((void)(it), (void)(iterations), true)
#endif

// ---- rigid bundles: entry j of a member's rotation in its object points (rigid_layout.h), and the divisor of the means (rigid_pose.h) --
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 19
#define RIGID_MEMBER_R(R, j) ((void)(R), ((j) % 4 == 0 ? 1.0 : 0.0))
#else
#define RIGID_MEMBER_R(R, j) ((R)[j])
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 20
#define RIGID_NPTS(n) ((void)(n), 4.0)
#else
#define RIGID_NPTS(n) (n)
#endif

// ---- camera rigs (rig_pose.h, kernels_rig.h): the ray origin as the translation statement sees it, entry (i, k) of the matrix that
// ---- carries a viewing ray into the rig frame (Rc^T), and the number of observation slots a solve fills ------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 46
#define RIG_T_ORIGIN(o) ((void)(o), 0.0)
#else
#define RIG_T_ORIGIN(o) (o)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 47
#define RIG_RAY_R(R, i, k) ((R)[3 * (i) + (k)])
#else
#define RIG_RAY_R(R, i, k) ((R)[3 * (k) + (i)])
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 48
#define RIG_SLOT_CUT 63u
#else
#define RIG_SLOT_CUT 64u
#endif

// ---- pose_covariance.h: the skew term of J_u; the pose the second quad of k_pose_refine<true> evaluates at (own: its chain's entry,
// ---- lane0: the lane of the record's first quad); the object point of a rigid bundle's covariance (p: the point, c: p - mean p) ----------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 25
#define POSE_COV_JU_SKEW(b) ((void)(b), 0.0)
#else
#define POSE_COV_JU_SKEW(b) (b)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 26
#define POSE_COV_CHAIN1_AT(own, lane0) __shfl((own), (lane0))
#else
#define POSE_COV_CHAIN1_AT(own, lane0) ((void)(lane0), (own))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 27
#define RIGID_COV_POINT(p, c) ((void)(p), (c))
#else
#define RIGID_COV_POINT(p, c) ((void)(c), (p))
#endif

// ---- k_decode_wave: whether step k of `steps` of the normal search enters the sums (in: both reads lie inside the image), and whether
// ---- index oi replaces index bid at equal distance in the code scan's reduction -----------------------------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 21
#define DW_STEP_COUNTED(in, k, steps) ((void)(in), (k) < (steps))
#else
#define DW_STEP_COUNTED(in, k, steps) (in)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 22
#define DW_TIE_TAKES(oi, bid) ((oi) > (bid))
#else
#define DW_TIE_TAKES(oi, bid) ((oi) < (bid))
#endif
// ---- k_decode_wave: whether distance hd replaces a lane's own best in the code scan (the lane's codes come in ascending index); the
// ---- lanes whose bits enter the quarter turn's ballot; the valid bit of a border sample stored at index sidx -----------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 56
#define DW_LANE_TAKES(hd, best) ((hd) <= (best))
#else
#define DW_LANE_TAKES(hd, best) ((hd) < (best))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 57
#define DW_TURN_LANE(lane, nbits) ((lane) < (nbits) && (lane) < 63)
#else
#define DW_TURN_LANE(lane, nbits) ((lane) < (nbits))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 58
#define DW_SAMPLE_FLAG(flag, sidx) ((sidx) >= 64 ? (flag) & ~1 : (flag))
#else
#define DW_SAMPLE_FLAG(flag, sidx) (flag)
#endif

// ---- k_reconcile: a containment test of quads_overlap_dev, and "margin a goes before margin b" of det_before_dev ------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 23
#define QO_CONTAINMENT(inside) ((void)(inside), false)
#else
#define QO_CONTAINMENT(inside) (inside)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 24
#define DET_MARGIN_BEFORE(a, b) ((a) < (b))
#else
#define DET_MARGIN_BEFORE(a, b) ((a) > (b))
#endif

// ---- k_points -----------------------------------------------------------------------------------------------------------
#ifdef AMDAT_FQ_PROFILE   // prof[0..5]: tile load, emission tests + scan, list, block table, stores, frame table
#define PT_HOOKS_DECL unsigned long long t_prev_ = prof ? __builtin_readcyclecounter() : 0ull;
#define PT_TICK(slot) if (prof && threadIdx.x == 0) { const unsigned long long now_ = __builtin_readcyclecounter(); atomicAdd(&prof[slot], now_ - t_prev_); t_prev_ = now_; }
#else
#define PT_HOOKS_DECL (void)prof;
#define PT_TICK(slot)
#endif
#ifdef AMDAT_PT_STOP      // `keep_live` is a store that keeps the results of the phases so far alive
#define PT_STOP_AT(n, keep_live) if (AMDAT_PT_STOP == (n) && P.max_nmaxima == 10) { keep_live; return; }
#else
#define PT_STOP_AT(n, keep_live)
#endif

// ---- k_cluster_select: the cluster-size cap of a frame (fd: its FrameDesc) ----------------------------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 6
#define SEL_CLUSTER_CAP(fd, P) ((void)(fd), (P).max_cluster_points)
#else
#define SEL_CLUSTER_CAP(fd, P) ((fd).max_cluster_points)
#endif

// ---- k_fit_quads --------------------------------------------------------------------------------------------------------
#ifdef AMDAT_FQ_TIMELINE
#define FQ_TIMELINE_GLOBALS                                                                                             \
  __device__ unsigned long long g_pf_span[4];   /* prefilter: earliest block start, latest block end; k_scatter's latest end; k_quad_finish's earliest start */ \
  __device__ unsigned long long g_fq_tl[1 << 16][2];                                                                    \
  __device__ unsigned int g_fq_ph[1 << 16][8];   /* wall-clock ticks (10 ns) per phase of the same cluster */           \
  __device__ unsigned int g_fq_tl_n;
#else
#define FQ_TIMELINE_GLOBALS
#endif

#if defined(AMDAT_FQ_PROFILE)
// points of the clusters that the test after the first walk rejects (k = 2): prof[40 + 4 * class + k] (the launch passes
// prof + 8 * class)
#define FQ_HOOKS_DECL unsigned long long t_prev_ = prof ? __builtin_readcyclecounter() : 0ull;
#define FQ_TICK(slot)                                                                  \
  if (prof && tid == 0) {                                                              \
    const unsigned long long now_ = __builtin_readcyclecounter();                      \
    atomicAdd(&prof[slot], now_ - t_prev_);                                            \
    t_prev_ = now_;                                                                    \
  }
#define FQ_COUNT(k, n) if (prof && tid == 0) atomicAdd(&prof[40 - 4 * ((NT == 64) ? 0 : (NT == 128) ? 1 : (NT == 256) ? 2 : (NT == 512) ? 3 : 4) + (k)], (unsigned long long)(n));
#define FQ_TL_NEXT_CLUSTER()
#define FQ_TL_SIZE(sz)
#elif defined(AMDAT_FQ_TIMELINE)
#define FQ_HOOKS_DECL (void)prof; unsigned long long tl_t0_ = 0, tl_prev_ = 0; unsigned int tl_sz_ = 0; unsigned int tl_ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define FQ_TICK(slot) if (tid == 0) { const unsigned long long now_ = wall_clock64(); tl_ph_[slot] += (unsigned int)(now_ - tl_prev_); tl_prev_ = now_; }
#define FQ_COUNT(k, n)
#define FQ_TL_NEXT_CLUSTER()                                                                                            \
  if (tid == 0) {                                                                                                       \
    const unsigned long long now_ = wall_clock64();                                                                     \
    if (tl_sz_) {                                                                                                       \
      const unsigned int k_ = atomicAdd(&g_fq_tl_n, 1u);                                                                \
      if (k_ < (1u << 16)) {                                                                                            \
        g_fq_tl[k_][0] = tl_t0_; g_fq_tl[k_][1] = ((now_ - tl_t0_) << 32) | ((unsigned long long)NT << 20) | (unsigned long long)tl_sz_; \
        for (int j_ = 0; j_ < 8; j_++) g_fq_ph[k_][j_] = tl_ph_[j_];                                                    \
      }                                                                                                                 \
    }                                                                                                                   \
    tl_t0_ = now_; tl_prev_ = now_; tl_sz_ = 0;                                                                         \
    for (int j_ = 0; j_ < 8; j_++) tl_ph_[j_] = 0;                                                                      \
  }
#define FQ_TL_SIZE(sz) tl_sz_ = (unsigned int)(sz);
#else
#define FQ_HOOKS_DECL (void)prof;
#define FQ_TICK(slot)
#define FQ_COUNT(k, n)
#define FQ_TL_NEXT_CLUSTER()
#define FQ_TL_SIZE(sz)
#endif
#ifdef AMDAT_FQ_STOP
#define FQ_STOP_AT(n) if (AMDAT_FQ_STOP == (n) && P.max_nmaxima == 10) continue;
#else
#define FQ_STOP_AT(n)
#endif

#ifdef AMDAT_FQ_TIMELINE
#define TL_MARK_MIN(slot) if (threadIdx.x == 0) atomicMin(&g_pf_span[slot], wall_clock64());
#define TL_MARK_MAX(slot) if (threadIdx.x == 0) atomicMax(&g_pf_span[slot], wall_clock64());
#else
#define TL_MARK_MIN(slot)
#define TL_MARK_MAX(slot)
#endif
// ---- k_fit_prefilter: prof[60..63] = box + dot, sector sums, scan + 32-sector test, 64-sector test --------------------
#ifdef AMDAT_FQ_PROFILE
#define PF_HOOKS_DECL unsigned long long t_prev_ = prof ? __builtin_readcyclecounter() : 0ull;
#define PF_TICK(slot) if (prof && tid == 0) { const unsigned long long now_ = __builtin_readcyclecounter(); atomicAdd(&prof[slot], now_ - t_prev_); t_prev_ = now_; }
#else
#define PF_HOOKS_DECL (void)prof;
#define PF_TICK(slot)
#endif

// ---- the SOUND early exits of the quad fit can be compiled out, one by one, to show that no result depends on them
// (-DAMDAT_FQ_NO_EARLY_EXIT, -DAMDAT_FQ_NO_PREFILTER: the A/B builds give the same bytes) ----------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 3
#define PF_MUT_EXTRA_SECTOR(nt) ((nt) == 64 ? 1 : 0)
#else
#define PF_MUT_EXTRA_SECTOR(nt) 0
#endif
// the line-fit limit the group test after the first walk is handed (NT: the instance's threads)
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 7
#define FQ_GROUP_TEST_MSE(NT, mse) (((NT) == 256 || (NT) == 1024) ? 0.25 * (mse) : (mse))
#else
#define FQ_GROUP_TEST_MSE(NT, mse) (mse)
#endif
// what the last wave of a chunk adds to the general sweep's running carry (t: its totals, a U128)
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 8
#define FQ_CARRY_LAST_WAVE(t) u128_add((t), (t))
#else
#define FQ_CARRY_LAST_WAVE(t) (t)
#endif
#ifdef AMDAT_FQ_NO_EARLY_EXIT
#define FQ_SOUND_EXIT_AFTER_WALK1 0
#else
#define FQ_SOUND_EXIT_AFTER_WALK1 1
#endif
#ifdef AMDAT_FQ_NO_PREFILTER
#define FQ_SOUND_EXIT_PREFILTER 0
#else
#define FQ_SOUND_EXIT_PREFILTER 1
#endif

// ---- raw formats (raw_formats.h, kernels_raw.h): the reflected index beyond the far border; which green sites have their red
// ---- neighbours east and west (yr: the site's row is a red row); the saturation of a shifted 16-bit sample; the x phase an instance
// ---- of BPS bytes per sample takes ---------------------------------------------------------------------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 49
#define RAW_REFLECT_FAR(i, n) ((n) - 1)
#else
#define RAW_REFLECT_FAR(i, n) (2 * ((n) - 1) - (i))
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 50
#define RAW_GREEN_RED_HORIZONTAL(yr) true
#else
#define RAW_GREEN_RED_HORIZONTAL(yr) (yr)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 51
#define RAW_SATURATE(s) ((s) & 255u)
#else
#define RAW_SATURATE(s) ((s) < 255u ? (s) : 255u)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 52
#define RAW_XPHASE(BPS, px) ((BPS) == 2 ? 0u : (px))
#else
#define RAW_XPHASE(BPS, px) (px)
#endif

// ---- the tag table (tag_table.h): where the binary search over n keys ends; whether the wildcard is consulted first; the size
// ---- k_pose_refine takes for a record (handle: P.tag_size, looked_up: the table's) -------------------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 53
#define TT_SEARCH_END(n) ((n) > 0u ? (n) - 1u : 0u)
#else
#define TT_SEARCH_END(n) (n)
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 54
#define TT_WILDCARD_FIRST true
#else
#define TT_WILDCARD_FIRST false
#endif
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 55
#define PR_TAG_SIZE(handle, looked_up) ((void)(looked_up), (handle))
#else
#define PR_TAG_SIZE(handle, looked_up) ((void)(handle), (looked_up))
#endif

// ---- launch sequence (detector.hip) ---------------------------------------------------------------------------------------
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 1
#define FQ_SKIP_PREFILTER() 0
#define FQ_SKIP_CLASS(c) ((c) < FQ_C0)
#elif defined(AMDAT_FQ_SKIP)
#define FQ_SKIP_PREFILTER() (((AMDAT_FQ_SKIP) >> 5) & 1)
#define FQ_SKIP_CLASS(c) ((c) >= FQ_C0 && (((AMDAT_FQ_SKIP) >> ((c) - FQ_C0)) & 1))
#else
#define FQ_SKIP_PREFILTER() 0
#define FQ_SKIP_CLASS(c) 0
#endif

// the parameter block of the decode launch (filt: the submission runs the quad_sigma filter)
#if defined(AMDAT_MUTATE) && AMDAT_MUTATE == 5
#define DECODE_PARAMS(P, filt) [&] { DetParams q_ = (P); if ((filt) && q_.decimate > 1) q_.refine_edges = 0; return q_; }()
#else
#define DECODE_PARAMS(P, filt) (P)
#endif
