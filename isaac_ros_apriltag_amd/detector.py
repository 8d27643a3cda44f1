"""Python host-side view of the detector handle (thin; all work happens behind the C ABI).

Mirrors the call shape the reference node uses on cuAprilTags (reference
isaac_ros_apriltag/src/apriltag_node.cpp:450-452 create, :491-493 detect, :556 destroy): create once
per (width, height, family, intrinsics, size); detect is host-synchronous; destroy in close().
"""
import ctypes as C

import numpy as np

from . import capi


def _as_images(frames, width, height, channels=1, per_frame=False, sample_bytes=1):
    """frames: torch uint8 CUDA tensor [n,H,W] / [H,W] (colour: [n,H,W,C] / [H,W,C], interleaved), or a list of such tensors,
    or a list of (dev_ptr, pitch) pairs or (dev_ptr, pitch, width, height) tuples.  width, height: the handle's size, which a
    two-element pair means; with per_frame (the handle's per-frame sizes mode) a tensor brings its own size, from its shape.
    A four-element tuple always names its own size -- a window is (pointer to its first pixel, the full image's pitch, its
    width, its height).  sample_bytes 2 (the 16-bit encodings): tensors of a 16-bit integer type, the pitch their row stride x 2;
    a tuple's pitch is in bytes as ever.  Returns (ctypes array, keepalive)."""
    items = []
    if sample_bytes != 1:
        for t in ([frames] if hasattr(frames, "data_ptr") else [f for f in frames if hasattr(f, "data_ptr")]):
            assert t.element_size() == sample_bytes, "expected %d-byte samples" % sample_bytes
    if hasattr(frames, "data_ptr"):
        t = frames
        if t.dim() == (2 if channels == 1 else 3):
            t = t.unsqueeze(0)
        if channels == 1:
            assert t.dim() == 3 and t.stride(2) == 1, "expected [n,H,W] mono8 with unit pixel stride"
        else:
            assert t.dim() == 4 and t.shape[3] == channels and t.stride(3) == 1 and t.stride(2) == channels, "expected [n,H,W,C] interleaved"
        w, h = (int(t.shape[2]), int(t.shape[1])) if per_frame else (width, height)
        for i in range(t.shape[0]):
            items.append((t[i].data_ptr(), t.stride(1) * sample_bytes, w, h))
    else:
        for f in frames:
            if hasattr(f, "data_ptr"):
                if channels == 1:
                    assert f.dim() == 2 and f.stride(1) == 1
                else:
                    assert f.dim() == 3 and f.shape[2] == channels and f.stride(2) == 1 and f.stride(1) == channels
                w, h = (int(f.shape[1]), int(f.shape[0])) if per_frame else (width, height)
                items.append((f.data_ptr(), f.stride(0) * sample_bytes, w, h))
            elif len(f) == 4:
                items.append((int(f[0]), int(f[1]), int(f[2]), int(f[3])))
            else:
                items.append((int(f[0]), int(f[1]), width, height))
    arr = (capi.ImageInput * len(items))()
    for i, (ptr, pitch, w, h) in enumerate(items):
        arr[i].width, arr[i].height, arr[i].dev_ptr, arr[i].pitch = w, h, ptr, pitch
    return arr, frames


class AprilTagDetector:
    def __init__(self, width, height, families=("tag36h11",), decimate=1, intrinsics=None, tag_size=0.22, max_batch=1,
                 tile_size=4, device=-1, refine_edges=True, quad_sigma=0.0, per_frame_sizes=False, rectification=None, resize=None,
                 bundles=None, pose_refinement=0, bundles_ex=None, pose_covariance=0.0, corner_undistortion=None, rig=None, raw_shift=None, tags=None,
                 listed_only=False, **caps):
        L = capi.lib()
        cfg = capi.Config()
        L.amdAprilTagsDefaultConfig(C.byref(cfg), width, height)
        cfg.tile_size = tile_size
        cfg.decimate = decimate
        cfg.num_families = len(families)
        for i, f in enumerate(families):
            e = f if isinstance(f, int) else L.amdAprilTagsFamilyFromName(f.encode())
            if e < 0:
                raise capi.AprilTagsError("family lookup %r" % (f,), 2)
            cfg.families[i] = e
        if intrinsics is not None:
            cfg.intrinsics = capi.Intrinsics(*[float(v) for v in intrinsics])
        cfg.tag_size = tag_size
        cfg.max_batch = max_batch
        cfg.refine_edges = 1 if refine_edges else 0
        cfg.device = device
        for k, v in caps.items():
            if not hasattr(cfg, k):
                raise AttributeError(k)
            setattr(cfg, k, v)
        self.families = [f if isinstance(f, str) else capi.family_info(f)["name"] for f in families]
        self.width, self.height, self.decimate, self.max_batch = width, height, decimate, max_batch
        self._h = C.c_void_p()
        capi._check("amdCreateAprilTagsDetectorEx", L.amdCreateAprilTagsDetectorEx(C.byref(self._h), C.byref(cfg)))
        self._L = L
        self.per_frame_sizes = False
        self.resizing = False
        self.nbundles = 0
        self.nbundles_ex = 0
        self.pose_refinement = 0
        self.pose_covariance = 0.0
        try:
            if quad_sigma:
                self.set_quad_sigma(quad_sigma)
            if per_frame_sizes:
                self.set_per_frame_sizes(True)
            if rectification:
                self.set_rectification(rectification)
            if resize:
                self.set_resize(resize)
            if corner_undistortion:
                self.set_corner_undistortion(corner_undistortion)
            if bundles:
                self.set_bundles(bundles)
            if bundles_ex:
                self.set_bundles_ex(bundles_ex)
            if pose_refinement:
                self.set_pose_refinement(pose_refinement)
            if pose_covariance:
                self.set_pose_covariance(pose_covariance)
            if rig:
                self.set_rig(rig)
            if raw_shift is not None:
                self.set_raw_shift(raw_shift)
            if tags:
                self.set_tag_table(tags, listed_only)
        except Exception:
            self.close()
            raise

    def set_quad_sigma(self, sigma):
        """quad_sigma (amdAprilTagsSetQuadSigma): blur (> 0) or sharpen (< 0) of the working image; takes effect with the next submission."""
        capi._check("amdAprilTagsSetQuadSigma", self._L.amdAprilTagsSetQuadSigma(self._h, float(sigma)))

    def set_raw_shift(self, shift):
        """amdAprilTagsSetRawShift: the sample of the 16-bit encodings ("mono16", "bayer_*16") is min(255, s >> shift); 0 .. 8, default 8,
        4 for a sensor with 12 significant bits.  Takes effect with the next submission."""
        capi._check("amdAprilTagsSetRawShift", self._L.amdAprilTagsSetRawShift(self._h, int(shift)))

    def set_tag_table(self, tags, listed_only=False):
        """amdAprilTagsSetTagTable: tags is a list of (family, id, size) -- family a name of the handle's list or an index into it; id an
        int, "*" for every id of the family without an entry of its own, or an inclusive (first, last) range; size the tag's edge in
        metres, 0 for the handle's tag_size.  Every following submission reports each tag's pose, undistorted twin, refined pose and
        covariance at its own size; with listed_only, tags that the table does not list are not reported at all (members of bundles
        included: list them).  None or [] turns the table off."""
        arr = capi.tag_entries(tags, self.families)
        capi._check("amdAprilTagsSetTagTable",
                    self._L.amdAprilTagsSetTagTable(self._h, len(arr) if arr is not None else 0, arr, 1 if (listed_only and arr is not None) else 0))

    def set_per_frame_sizes(self, enable=True):
        """amdAprilTagsSetPerFrameSizes: every frame of a submission brings its own size, up to the handle's (width, height are then
        the largest frame); tensors are taken at their shape, (dev_ptr, pitch, width, height) tuples as they say."""
        capi._check("amdAprilTagsSetPerFrameSizes", self._L.amdAprilTagsSetPerFrameSizes(self._h, 1 if enable else 0))
        self.per_frame_sizes = bool(enable)

    def set_rectification(self, models):
        """amdAprilTagsSetRectification[Ex]: models is a list of (K, D, Knew) -- a plumb_bob camera -- or (K, D, Knew, model_name, R)
        with model_name "plumb_bob", "rational_polynomial" or "equidistant" and R the CameraInfo's rectification rotation (None: the
        identity).  Frame i of every following submission is undistorted with models[i % len(models)] inside the submission and
        detected there; None or [] turns it off.  The pose intrinsics stay the caller's: pass Knew's fx, fy, cx, cy (R does not enter
        the pose: it is reported in the rectified camera's frame).  A list of 3-tuples alone goes through amdAprilTagsSetRectification."""
        models = list(models or [])
        if any(len(m) != 3 for m in models):
            arr = capi.camera_models_ex(models)
            capi._check("amdAprilTagsSetRectificationEx", self._L.amdAprilTagsSetRectificationEx(self._h, len(arr), arr))
            return
        arr = capi.camera_models(models)
        capi._check("amdAprilTagsSetRectification", self._L.amdAprilTagsSetRectification(self._h, len(arr) if arr is not None else 0, arr))

    def set_resize(self, sizes):
        """amdAprilTagsSetResize: sizes is a list of (width, height) -- frame i of every following submission, whatever its own size, is
        resized to sizes[i % len(sizes)] inside the submission (through the rectification where that is on) and detected there; None
        or [] turns it off.  Tensors are then taken at their shape.  The pose intrinsics stay the caller's: scale them by dw / sw and
        dh / sh."""
        arr = capi.sizes(sizes)
        capi._check("amdAprilTagsSetResize", self._L.amdAprilTagsSetResize(self._h, len(arr) if arr is not None else 0, arr))
        self.resizing = arr is not None

    def set_bundles(self, bundles):
        """amdAprilTagsSetBundles: bundles is a list of {"name", "members": [(family_index, id, x, y, size)], "max_hamming",
        "min_decision_margin", "min_tags"} (capi.bundles) -- planar boards whose pose every following submission solves per frame from
        all kept records, behind the detector; None or [] turns it off.  bundle_poses(n) hands out the records."""
        arr = capi.bundles(bundles)
        capi._check("amdAprilTagsSetBundles", self._L.amdAprilTagsSetBundles(self._h, len(arr) if arr is not None else 0, arr))
        self.nbundles = len(arr) if arr is not None else 0
        if self.nbundles:
            self.nbundles_ex = 0   # (one kind is on at a time: the later call holds)

    def bundle_poses(self, n):
        """amdAprilTagsGetBundlePoses: the bundle records of the first n frames of the last completed submission, a list per frame of
        {"bundle", "status", "ntags", "nskipped", "R" (3x3), "t", "sq_err_sum"} in the order of set_bundles."""
        out = (capi.BundlePose * max(n * self.nbundles, 1))()
        capi._check("amdAprilTagsGetBundlePoses", self._L.amdAprilTagsGetBundlePoses(self._h, out, n))
        return [[{"bundle": int(r.bundle), "status": int(r.status), "ntags": int(r.ntags), "nskipped": int(r.nskipped),
                  "R": np.array(list(r.R)).reshape(3, 3), "t": np.array(list(r.t)), "sq_err_sum": float(r.sq_err_sum)}
                 for r in out[f * self.nbundles:(f + 1) * self.nbundles]] for f in range(n)]

    def set_bundles_ex(self, bundles):
        """amdAprilTagsSetBundlesEx: bundles is a list of {"name", "iterations", "members": [(family_index, id, R, t, size)],
        "max_hamming", "min_decision_margin", "min_tags"} (capi.bundles_ex) -- rigid 3-D bundles (cubes, rigs, boards with turned tags),
        every member with its pose (R, t) in the bundle frame, solved per frame as one rigid body from all kept records; None or []
        turns it off.  Turning it on turns set_bundles' planar kind off.  bundle_poses_ex(n) hands out the records."""
        arr = capi.bundles_ex(bundles)
        capi._check("amdAprilTagsSetBundlesEx", self._L.amdAprilTagsSetBundlesEx(self._h, len(arr) if arr is not None else 0, arr))
        self.nbundles_ex = len(arr) if arr is not None else 0
        if self.nbundles_ex:
            self.nbundles = 0

    def bundle_poses_ex(self, n):
        """amdAprilTagsGetBundlePosesEx: the rigid bundle records of the first n frames of the last completed submission, a list per
        frame of {"bundle", "status", "ntags", "nskipped", "seed", "chosen", "R" (3x3), "t", "err", "sq_err_sum", "R_alt", "t_alt",
        "err_alt", "sq_err_sum_alt"} in the order of set_bundles_ex."""
        out = (capi.BundlePoseEx * max(n * self.nbundles_ex, 1))()
        capi._check("amdAprilTagsGetBundlePosesEx", self._L.amdAprilTagsGetBundlePosesEx(self._h, out, n))
        return [[{"bundle": int(r.bundle), "status": int(r.status), "ntags": int(r.ntags), "nskipped": int(r.nskipped), "seed": int(r.seed),
                  "chosen": int(r.chosen), "R": np.array(list(r.R)).reshape(3, 3), "t": np.array(list(r.t)), "err": float(r.err),
                  "sq_err_sum": float(r.sq_err_sum), "R_alt": np.array(list(r.R_alt)).reshape(3, 3), "t_alt": np.array(list(r.t_alt)),
                  "err_alt": float(r.err_alt), "sq_err_sum_alt": float(r.sq_err_sum_alt)}
                 for r in out[f * self.nbundles_ex:(f + 1) * self.nbundles_ex]] for f in range(n)]

    def set_rig(self, cams):
        """amdAprilTagsSetRig: cams is a list of (R, t), one per camera of a calibrated rig, the RIG frame in the CAMERA frame
        (X_cam = R X_rig + t).  Every following submission in which set_bundles_ex is on solves one pose per group of frames (the
        cameras of one instant: set_rig_slots) and rigid bundle, in the rig frame, over the tags of all the group's cameras at once;
        the per-frame records stay as they are.  None or [] turns it off.  rig_bundle_poses(ngroups) hands out the records."""
        arr = capi.rig_cameras(cams)
        capi._check("amdAprilTagsSetRig", self._L.amdAprilTagsSetRig(self._h, len(arr) if arr is not None else 0, arr))

    def set_rig_slots(self, slots):
        """amdAprilTagsSetRigSlots: slots is a list of (group, camera) for batch slots 0 .. len(slots) - 1 of the submissions that
        follow (camera capi.RIG_NO_CAMERA: the slot belongs to no group); the slots beyond, and all of them for None or [], follow
        the default map: camera i % ncams of group i / ncams."""
        slots = list(slots or [])
        arr = (capi.RigSlot * max(len(slots), 1))()
        for i, (g, c) in enumerate(slots):
            arr[i].group, arr[i].camera = int(g), int(c)
        capi._check("amdAprilTagsSetRigSlots", self._L.amdAprilTagsSetRigSlots(self._h, len(slots), arr if slots else None))

    def rig_bundle_poses(self, ngroups):
        """amdAprilTagsGetRigBundlePoses: the rig records of the first ngroups groups of the last completed submission, a list per
        group of {"group", "bundle", "status", "nobs", "nskipped", "ndropped", "ncams", "seed_frame", "seed", "chosen", "R" (3x3), "t",
        "err", "sq_err_sum", "R_alt", "t_alt", "err_alt", "sq_err_sum_alt"} in the order of set_bundles_ex."""
        nb = self.nbundles_ex
        out = (capi.RigBundlePose * max(ngroups * nb, 1))()
        capi._check("amdAprilTagsGetRigBundlePoses", self._L.amdAprilTagsGetRigBundlePoses(self._h, out, ngroups))
        ints = ("group", "bundle", "status", "nobs", "nskipped", "ndropped", "ncams", "seed_frame", "seed", "chosen")
        return [[dict({k: int(getattr(r, k)) for k in ints}, R=np.array(list(r.R)).reshape(3, 3), t=np.array(list(r.t)), err=float(r.err),
                      sq_err_sum=float(r.sq_err_sum), R_alt=np.array(list(r.R_alt)).reshape(3, 3), t_alt=np.array(list(r.t_alt)),
                      err_alt=float(r.err_alt), sq_err_sum_alt=float(r.sq_err_sum_alt))
                 for r in out[g * nb:(g + 1) * nb]] for g in range(ngroups)]

    def set_pose_refinement(self, iterations):
        """amdAprilTagsSetPoseRefinement: every following submission refines the records it hands out by orthogonal iteration from two
        starts, `iterations` steps each (1 .. 200; upstream's estimate_tag_pose runs 50); 0 turns it off.  The detection records keep the
        homography pose; refined_poses(n) hands out the refined ones."""
        capi._check("amdAprilTagsSetPoseRefinement", self._L.amdAprilTagsSetPoseRefinement(self._h, int(iterations)))
        self.pose_refinement = int(iterations)

    def refined_poses(self, n):
        """amdAprilTagsGetRefinedPoses: the refined poses of the first n frames of the last completed submission, a list per frame,
        aligned by index with the frame's detections, of {"status", "chosen", "R" (3x3), "t", "err", "R_alt", "t_alt", "err_alt",
        "err_homography"}."""
        out = []
        for f in range(n):
            cnt = C.c_uint32(0)
            probe = (capi.RefinedPose * 1)()
            rc = self._L.amdAprilTagsGetRefinedPoses(self._h, f, probe, 0, C.byref(cnt))   # the count (refused for its capacity when > 0)
            if rc and cnt.value == 0:
                capi._check("amdAprilTagsGetRefinedPoses", rc)
            arr = (capi.RefinedPose * max(cnt.value, 1))()
            capi._check("amdAprilTagsGetRefinedPoses", self._L.amdAprilTagsGetRefinedPoses(self._h, f, arr, cnt.value, C.byref(cnt)))
            out.append([{"status": int(r.status), "chosen": int(r.chosen), "R": np.array(list(r.R)).reshape(3, 3), "t": np.array(list(r.t)),
                         "err": float(r.err), "R_alt": np.array(list(r.R_alt)).reshape(3, 3), "t_alt": np.array(list(r.t_alt)),
                         "err_alt": float(r.err_alt), "err_homography": float(r.err_homography)} for r in arr[:cnt.value]])
        return out

    def set_pose_covariance(self, sigma_px):
        """amdAprilTagsSetPoseCovariance: every pose that set_pose_refinement and set_bundles_ex hand out comes with a first-order
        6 x 6 covariance in ROS' PoseWithCovariance order (x, y, z, rotation about x, y, z; camera optical frame), for independent corner
        noise of standard deviation sigma_px, which is the caller's figure; 0 turns it off.  refined_pose_covariances(n) and
        bundle_pose_covariances_ex(n) hand out the records."""
        capi._check("amdAprilTagsSetPoseCovariance", self._L.amdAprilTagsSetPoseCovariance(self._h, float(sigma_px)))
        self.pose_covariance = float(sigma_px)

    def refined_pose_covariances(self, n):
        """amdAprilTagsGetRefinedPoseCovariances: the covariance records beside refined_poses(n), a numpy array of capi.POSE_COV_DTYPE
        per frame ("cov", "cov_alt" (6x6), "sq_err_sum", "sq_err_sum_alt", "valid": bit 0 cov, bit 1 cov_alt)."""
        out = []
        for f in range(n):
            cnt = C.c_uint32(0)
            probe = (capi.PoseCovariance * 1)()
            rc = self._L.amdAprilTagsGetRefinedPoseCovariances(self._h, f, probe, 0, C.byref(cnt))   # the count (refused for its capacity when > 0)
            if rc and cnt.value == 0:
                capi._check("amdAprilTagsGetRefinedPoseCovariances", rc)
            arr = np.zeros(max(cnt.value, 1), dtype=capi.POSE_COV_DTYPE)
            capi._check("amdAprilTagsGetRefinedPoseCovariances", self._L.amdAprilTagsGetRefinedPoseCovariances(
                self._h, f, arr.ctypes.data_as(C.POINTER(capi.PoseCovariance)), cnt.value, C.byref(cnt)))
            out.append(arr[:cnt.value])
        return out

    def bundle_pose_covariances_ex(self, n):
        """amdAprilTagsGetBundlePoseCovariancesEx: the covariance records beside bundle_poses_ex(n), a numpy array of
        capi.POSE_COV_DTYPE of shape (n, bundles)."""
        arr = np.zeros(max(n * self.nbundles_ex, 1), dtype=capi.POSE_COV_DTYPE)
        capi._check("amdAprilTagsGetBundlePoseCovariancesEx", self._L.amdAprilTagsGetBundlePoseCovariancesEx(
            self._h, arr.ctypes.data_as(C.POINTER(capi.PoseCovariance)), n))
        return arr[:n * self.nbundles_ex].reshape(n, self.nbundles_ex)

    def set_corner_undistortion(self, models):
        """amdAprilTagsSetCornerUndistortion (raw-frame mode): models is a list of (K, D, Knew) or (K, D, Knew, model_name, R), as
        set_rectification takes them.  Frame i of every following submission is detected as it stands, and every record it keeps gets an
        undistorted twin under models[i % len(models)]: corners through the inverse of the camera model, the exact homography onto them,
        centre and pose from that.  The detection records keep the raw frame's values; undistorted_detections(n) hands out the twins, and
        bundle_poses, bundle_poses_ex, refined_poses and the covariances are computed from them.  Pass Knew's fx, fy, cx, cy as the pose
        intrinsics.  None or [] turns it off; refused while rectification is on."""
        arr = capi.camera_models_ex(list(models or []))
        capi._check("amdAprilTagsSetCornerUndistortion", self._L.amdAprilTagsSetCornerUndistortion(self._h, len(arr), arr))

    def undistorted_detections(self, n):
        """amdAprilTagsGetUndistortedDetections: the undistorted twins of the first n frames of the last completed submission, a list per
        frame, aligned by index with the frame's detections, of {"status" (capi.UNDISTORT_OK / UNDISTORT_INVALID), "H" (3x3), "center",
        "p" (4x2), "R" (3x3), "t"}; an invalid record's fields are all zero."""
        out = []
        for f in range(n):
            cnt = C.c_uint32(0)
            probe = (capi.UndistortedDetection * 1)()
            rc = self._L.amdAprilTagsGetUndistortedDetections(self._h, f, probe, 0, C.byref(cnt))   # the count (refused for its capacity when > 0)
            if rc and cnt.value == 0:
                capi._check("amdAprilTagsGetUndistortedDetections", rc)
            arr = (capi.UndistortedDetection * max(cnt.value, 1))()
            capi._check("amdAprilTagsGetUndistortedDetections",
                        self._L.amdAprilTagsGetUndistortedDetections(self._h, f, arr, cnt.value, C.byref(cnt)))
            out.append([{"status": int(r.status), "H": np.array(list(r.H)).reshape(3, 3), "center": np.array(list(r.c)),
                         "p": np.array([[r.p[i][0], r.p[i][1]] for i in range(4)]), "R": np.array(list(r.R)).reshape(3, 3),
                         "t": np.array(list(r.t))} for r in arr[:cnt.value]])
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.amdAprilTagsDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- detection --------------------------------------------------------------------------------
    def detect_batch_ex(self, frames, max_dets=64, intrinsics=None, stream=None, encoding="mono8"):
        """encoding != "mono8": frames are interleaved colour ([n,H,W,C]), or for the raw formats ("bayer_rggb8" .. "bayer_grbg16",
        "mono16") one sample per pixel ([n,H,W], uint8 or a 16-bit integer type), and go through amdAprilTagsDetectBatchColorEx."""
        imgs, keep = _as_images(frames, self.width, self.height, capi.ENC_CHANNELS[encoding], self.per_frame_sizes or self.resizing,
                                capi.ENC_SAMPLE_BYTES.get(encoding, 1))
        n = len(imgs)
        out = (capi.DetectionEx * (n * max_dets))()
        cnt = (C.c_uint32 * n)()
        intr = None
        if intrinsics is not None:
            intr = (capi.Intrinsics * n)(*[capi.Intrinsics(*[float(v) for v in k]) for k in intrinsics])
        if encoding == "mono8":
            capi._check("amdAprilTagsDetectBatchEx",
                        self._L.amdAprilTagsDetectBatchEx(self._h, n, imgs, intr, out, cnt, max_dets, stream))
        else:
            capi._check("amdAprilTagsDetectBatchColorEx",
                        self._L.amdAprilTagsDetectBatchColorEx(self._h, n, imgs, capi.ENCODINGS[encoding], intr, out, cnt, max_dets, stream))
        res = []
        for f in range(n):
            dets = []
            for i in range(cnt[f]):
                d = out[f * max_dets + i]
                dets.append({"family": self.families[d.family], "id": int(d.id), "hamming": int(d.hamming),
                             "decision_margin": float(d.decision_margin),
                             "H": np.array(list(d.H)).reshape(3, 3), "center": np.array(list(d.c)),
                             "p": np.array([[d.p[k][0], d.p[k][1]] for k in range(4)]),
                             "R": np.array(list(d.R)).reshape(3, 3), "t": np.array(list(d.t))})
            res.append(dets)
        return res

    # ---- prepared submissions: argument marshalling done once, the timed call is only the C ABI call ----
    def prepare(self, frames, max_dets=64, intrinsics=None, encoding="mono8"):
        imgs, keep = _as_images(frames, self.width, self.height, capi.ENC_CHANNELS[encoding], self.per_frame_sizes or self.resizing,
                                capi.ENC_SAMPLE_BYTES.get(encoding, 1))
        n = len(imgs)
        intr = None
        if intrinsics is not None:
            assert len(intrinsics) == n
            intr = (capi.Intrinsics * n)(*[capi.Intrinsics(*[float(v) for v in k]) for k in intrinsics])
        return {"imgs": imgs, "keep": keep, "n": n, "max_dets": max_dets, "intr": intr, "enc": capi.ENCODINGS[encoding],
                "out": (capi.DetectionEx * (n * max_dets))(), "cnt": (C.c_uint32 * n)()}

    def run_prepared(self, prep, stream=None):
        """One blocking amdAprilTagsDetectBatchEx call; results stay in prep['out'] / prep['cnt']."""
        if prep.get("enc", 0):
            capi._check("amdAprilTagsDetectBatchColorEx",
                        self._L.amdAprilTagsDetectBatchColorEx(self._h, prep["n"], prep["imgs"], prep["enc"], prep.get("intr"), prep["out"],
                                                               prep["cnt"], prep["max_dets"], stream))
            return
        capi._check("amdAprilTagsDetectBatchEx",
                    self._L.amdAprilTagsDetectBatchEx(self._h, prep["n"], prep["imgs"], prep.get("intr"), prep["out"],
                                                      prep["cnt"], prep["max_dets"], stream))

    def submit_prepared(self, prep, stream=None):
        """amdAprilTagsSubmitBatch: enqueues and returns; wait_prepared() collects (results in prep['out'] / prep['cnt'])."""
        if prep.get("enc", 0):
            capi._check("amdAprilTagsSubmitBatchColor",
                        self._L.amdAprilTagsSubmitBatchColor(self._h, prep["n"], prep["imgs"], prep["enc"], prep.get("intr"), prep["max_dets"], stream))
            return
        capi._check("amdAprilTagsSubmitBatch",
                    self._L.amdAprilTagsSubmitBatch(self._h, prep["n"], prep["imgs"], prep.get("intr"), prep["max_dets"], stream))

    def wait_prepared(self, prep):
        capi._check("amdAprilTagsWaitBatchEx", self._L.amdAprilTagsWaitBatchEx(self._h, prep["out"], prep["cnt"]))

    def unpack(self, prep):
        res = []
        out, cnt, max_dets = prep["out"], prep["cnt"], prep["max_dets"]
        for f in range(prep["n"]):
            dets = []
            for i in range(cnt[f]):
                d = out[f * max_dets + i]
                dets.append({"family": self.families[d.family], "id": int(d.id), "hamming": int(d.hamming),
                             "decision_margin": float(d.decision_margin),
                             "H": np.array(list(d.H)).reshape(3, 3), "center": np.array(list(d.c)),
                             "p": np.array([[d.p[k][0], d.p[k][1]] for k in range(4)]),
                             "R": np.array(list(d.R)).reshape(3, 3), "t": np.array(list(d.t))})
            res.append(dets)
        return res

    def detect_batch_raw(self, frames, max_tags=64, intrinsics=None, stream=None):
        """Returns (TagID ctypes array of n*max_tags, counts) -- the cuAprilTagsID_t-shaped records."""
        imgs, keep = _as_images(frames, self.width, self.height, 1, self.per_frame_sizes or self.resizing)
        n = len(imgs)
        out = (capi.TagID * (n * max_tags))()
        cnt = (C.c_uint32 * n)()
        intr = None
        if intrinsics is not None:
            intr = (capi.Intrinsics * n)(*[capi.Intrinsics(*[float(v) for v in k]) for k in intrinsics])
        capi._check("amdAprilTagsDetectBatch",
                    self._L.amdAprilTagsDetectBatch(self._h, n, imgs, intr, out, cnt, max_tags, stream))
        return out, [int(c) for c in cnt]

    def threshold_only(self, frames, stream=None, encoding="mono8"):
        imgs, keep = _as_images(frames, self.width, self.height, capi.ENC_CHANNELS[encoding], self.per_frame_sizes,
                                capi.ENC_SAMPLE_BYTES.get(encoding, 1))
        if encoding == "mono8":
            capi._check("amdAprilTagsThresholdOnly", self._L.amdAprilTagsThresholdOnly(self._h, len(imgs), imgs, stream))
        else:
            capi._check("amdAprilTagsThresholdOnlyColor",
                        self._L.amdAprilTagsThresholdOnlyColor(self._h, len(imgs), imgs, capi.ENCODINGS[encoding], stream))

    # ---- measurement / inspection ---------------------------------------------------------------------
    def set_profiling(self, enable=True):
        """True/1: HIP events per stage; 2: plus cycle counters inside the quad-fit kernel."""
        capi._check("amdAprilTagsSetProfiling", self._L.amdAprilTagsSetProfiling(self._h, int(enable)))

    def set_submission_path(self, path):
        """'auto' (by submission size), 'latency' or 'throughput': pins the launch set (parity tests; results never depend on it)."""
        code = {"auto": capi.PATH_AUTO, "latency": capi.PATH_LATENCY, "throughput": capi.PATH_THROUGHPUT}[path] if isinstance(path, str) else int(path)
        capi._check("amdAprilTagsDebugSetSubmissionPath", self._L.amdAprilTagsDebugSetSubmissionPath(self._h, code))

    def late_waits(self):
        return int(self._L.amdAprilTagsDebugLateWaits(self._h))

    def graph_replay(self):
        """(still capturing new launch graphs?, live cache entries, retired graphs) -- include/apriltag_amd_debug.h."""
        live, ret = C.c_uint32(), C.c_uint32()
        on = self._L.amdAprilTagsDebugGraphReplay(self._h, C.byref(live), C.byref(ret))
        return bool(on), int(live.value), int(ret.value)

    def last_graph_nodes(self):
        """Nodes of the captured graph the last submission replayed; 0: plain enqueues."""
        return int(self._L.amdAprilTagsDebugLastGraphNodes(self._h))

    def set_frame_skews(self, skews):
        """amdAprilTagsSetFrameSkews: K[0][1] of batch slots 0 .. len(skews) - 1 for the submissions that follow."""
        arr = (C.c_float * max(len(skews), 1))(*[float(v) for v in skews])
        capi._check("amdAprilTagsSetFrameSkews", self._L.amdAprilTagsSetFrameSkews(self._h, len(skews), arr))

    def last_submission_path(self):
        return {capi.PATH_AUTO: "none", capi.PATH_LATENCY: "latency", capi.PATH_THROUGHPUT: "throughput"}[
            self._L.amdAprilTagsDebugLastSubmissionPath(self._h)]

    def stage_ms(self):
        ms = (C.c_float * capi.NUM_STAGES)()
        capi._check("amdAprilTagsGetStageMs", self._L.amdAprilTagsGetStageMs(self._h, ms))
        return dict(zip(capi.stage_names(), [float(v) for v in ms]))

    def frame_flags(self, n):
        fl = (C.c_uint32 * n)()
        capi._check("amdAprilTagsGetFrameFlags", self._L.amdAprilTagsGetFrameFlags(self._h, fl, n))
        return [int(v) for v in fl]

    def mean_counts(self, n, sample=16):
        """Mean per-frame content counters of the last submission over `sample` evenly spaced frames."""
        idx = sorted(set(int(i) for i in np.linspace(0, n - 1, min(sample, n))))
        c = np.array([self.debug(i, capi.DBG_COUNTS)[:5] for i in idx], dtype=np.float64).mean(axis=0)
        return {"npoints_raw": float(c[0]), "nclusters": float(c[1]), "npoints_kept": float(c[2]), "nquads": float(c[3]),
                "ndets_raw": float(c[4])}

    def device_bytes(self):
        """Device memory the handle owns."""
        nb = C.c_size_t()
        capi._check("amdAprilTagsGetDeviceBytes", self._L.amdAprilTagsGetDeviceBytes(self._h, C.byref(nb)))
        return int(nb.value)

    def debug(self, frame, what):
        """amdAprilTagsDebugCopy; what: a capi.DBG_* selector, or "raw_gray" for capi.DBG_RAW_GRAY."""
        if what == "raw_gray":
            what = capi.DBG_RAW_GRAY
        nbytes = C.c_size_t()
        capi._check("amdAprilTagsDebugCopy", self._L.amdAprilTagsDebugCopy(self._h, frame, what, None, 0, C.byref(nbytes)))
        buf = np.empty(max(nbytes.value, 1), dtype=np.uint8)
        capi._check("amdAprilTagsDebugCopy",
                    self._L.amdAprilTagsDebugCopy(self._h, frame, what, buf.ctypes.data, buf.size, C.byref(nbytes)))
        buf = buf[:nbytes.value]
        if what in (capi.DBG_GRAY, capi.DBG_THRESH, capi.DBG_RECTIFIED, capi.DBG_RESIZED, capi.DBG_RAW_GRAY):
            return buf
        if what in (capi.DBG_LABEL, capi.DBG_CSIZE, capi.DBG_POINTS, capi.DBG_COUNTS):
            return buf.view(np.uint32)
        if what == capi.DBG_CLUSTERS:
            return buf.view(capi.CLUSTER_DTYPE)
        if what == capi.DBG_QUADS:
            return buf.view(capi.QUAD_DTYPE)
        if what == capi.DBG_DETS:
            return buf.view(capi.DET_DTYPE)
        return buf

    def debug_reconcile(self, records):
        """amdAprilTagsDebugReconcile: k_reconcile alone on `records` (capi.DET_DTYPE; at most max_detections of them); the kept records
        in their final order, R and t filled.  The last submission's stage buffers cannot be read afterwards."""
        rec = np.array(records, dtype=capi.DET_DTYPE, order="C", copy=True).reshape(-1)
        out = np.zeros(max(len(rec), 1), dtype=capi.DET_DTYPE)
        nout = C.c_uint32()
        capi._check("amdAprilTagsDebugReconcile",
                    self._L.amdAprilTagsDebugReconcile(self._h, len(rec), rec.ctypes.data, out.ctypes.data, len(out), C.byref(nout)))
        return out[:min(nout.value, len(out))].copy()

    def debug_undistort(self, records, model):
        """amdAprilTagsDebugUndistort: k_undistort_records alone on `records` (capi.DET_DTYPE; at most max_detections of them, taken as
        one frame's kept records in the order given) under model = (K, D, Knew) or (K, D, Knew, model_name, R).  Returns (public records:
        capi.UNDISTORTED_DTYPE, device twins: capi.DET_DTYPE).  The last submission's stage buffers cannot be read afterwards."""
        rec = np.array(records, dtype=capi.DET_DTYPE, order="C", copy=True).reshape(-1)
        cam = capi.camera_models_ex([model])
        out = np.zeros(max(len(rec), 1), dtype=capi.UNDISTORTED_DTYPE)
        twins = np.zeros(max(len(rec), 1), dtype=capi.DET_DTYPE)
        capi._check("amdAprilTagsDebugUndistort",
                    self._L.amdAprilTagsDebugUndistort(self._h, len(rec), rec.ctypes.data, cam, out.ctypes.data, twins.ctypes.data))
        return out[:len(rec)].copy(), twins[:len(rec)].copy()
