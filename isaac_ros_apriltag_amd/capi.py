"""ctypes binding of libapriltag_amd.so -- the C ABI declared in include/apriltag_amd.h.

The library is the product: there is no CPU fallback.  Importing this module without the built
library, or creating a detector without a HIP device, raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libapriltag_amd.so")

NUM_STAGES = 12
FAMILY_ENUM = {"tag36h11": 0, "tag25h9": 1, "tag16h5": 2}
SLOT_TAG36H10, SLOT_CUSTOM0 = 3, 4   # registrable slots: 3 (tag36h10: no built-in table) and 4..8
(DBG_GRAY, DBG_THRESH, DBG_LABEL, DBG_CSIZE, DBG_CLUSTERS, DBG_POINTS, DBG_QUADS, DBG_COUNTS) = range(8)
DBG_RECTIFIED = 9   # u8 W0 x H0: the frame's rectified plane (amdAprilTagsSetRectification)
DBG_RESIZED = 10    # u8 dw x dh: the frame's resized plane (amdAprilTagsSetResize)
DBG_RAW_GRAY = 12   # u8 w x h at the source size: the frame's converted plane (a submission of Bayer or 16-bit frames)
DBG_DETS = 11       # DET_DTYPE x min(ndets, max_detections): the frame's decoded records before reconcile, in no order
# the records of the stage buffers as numpy sees them (include/apriltag_amd_debug.h; DET_DTYPE is amdAprilTagsDetectionEx_t)
CLUSTER_DTYPE = np.dtype([("key", "<u8"), ("start", "<u4"), ("count", "<u4")])
QUAD_DTYPE = np.dtype([("p", "<f4", (4, 2)), ("reversed_border", "<i4"), ("pad", "<u4"), ("key", "<u8")])
DET_DTYPE = np.dtype([("family", "<i4"), ("id", "<i4"), ("hamming", "<i4"), ("decision_margin", "<f4"), ("H", "<f8", (9,)),
                      ("c", "<f8", (2,)), ("p", "<f8", (4, 2)), ("R", "<f8", (9,)), ("t", "<f8", (3,))])
FLAG_DETS_OVERFLOW = 0x10   # AMDAT_FLAG_DETS_OVERFLOW

STATUS = {0: "AMDAT_SUCCESS", 1: "AMDAT_INVALID_ARGUMENT", 2: "AMDAT_UNSUPPORTED", 3: "AMDAT_HIP_ERROR",
          4: "AMDAT_SIZE_MISMATCH", 5: "AMDAT_OUT_OF_MEMORY", 6: "AMDAT_BATCH_TOO_LARGE"}


class Intrinsics(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class ImageInput(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("dev_ptr", C.c_void_p), ("pitch", C.c_size_t)]


class CameraModel(C.Structure):
    """amdAprilTagsCameraModel_t: row-major 3x3 K and Knew, plumb_bob D = k1, k2, p1, p2, k3."""
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 5), ("Knew", C.c_double * 9)]


class CameraModelEx(C.Structure):
    """amdAprilTagsCameraModelEx_t: kind (DISTORTIONS), row-major 3x3 K, R and Knew, D in CameraInfo's order for the kind."""
    _fields_ = [("kind", C.c_uint32), ("reserved", C.c_uint32), ("K", C.c_double * 9), ("D", C.c_double * 8), ("R", C.c_double * 9),
                ("Knew", C.c_double * 9)]


class Size(C.Structure):
    """amdAprilTagsSize_t."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32)]


class BundleMember(C.Structure):
    """amdAprilTagsBundleMember_t: tag (family_index, id) with its centre (x, y) on the board plane and its border edge, in metres."""
    _fields_ = [("family_index", C.c_uint32), ("id", C.c_uint32), ("x", C.c_double), ("y", C.c_double), ("size", C.c_double)]


class Bundle(C.Structure):
    """amdAprilTagsBundle_t."""
    _fields_ = [("members", C.POINTER(BundleMember)), ("nmembers", C.c_uint32), ("max_hamming", C.c_uint32),
                ("min_decision_margin", C.c_float), ("min_tags", C.c_uint32), ("name", C.c_char * 32)]


class BundlePose(C.Structure):
    """amdAprilTagsBundlePose_t."""
    _fields_ = [("bundle", C.c_uint32), ("status", C.c_uint32), ("ntags", C.c_uint32), ("nskipped", C.c_uint32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("sq_err_sum", C.c_double)]


BUNDLE_SOLVED, BUNDLE_TOO_FEW_TAGS, BUNDLE_SINGULAR = 0, 1, 2
MAX_BUNDLES, MAX_BUNDLE_MEMBERS = 8, 1024


class BundleMemberEx(C.Structure):
    """amdAprilTagsBundleMemberEx_t: tag (family_index, id) with its pose (R row-major, t) in the bundle frame and its border edge."""
    _fields_ = [("family_index", C.c_uint32), ("id", C.c_uint32), ("R", C.c_double * 9), ("t", C.c_double * 3), ("size", C.c_double)]


class BundleEx(C.Structure):
    """amdAprilTagsBundleEx_t."""
    _fields_ = [("members", C.POINTER(BundleMemberEx)), ("nmembers", C.c_uint32), ("max_hamming", C.c_uint32),
                ("min_decision_margin", C.c_float), ("min_tags", C.c_uint32), ("iterations", C.c_uint32), ("name", C.c_char * 32)]


class BundlePoseEx(C.Structure):
    """amdAprilTagsBundlePoseEx_t."""
    _fields_ = [("bundle", C.c_uint32), ("status", C.c_uint32), ("ntags", C.c_uint32), ("nskipped", C.c_uint32), ("seed", C.c_uint32),
                ("chosen", C.c_uint32), ("R", C.c_double * 9), ("t", C.c_double * 3), ("err", C.c_double), ("sq_err_sum", C.c_double),
                ("R_alt", C.c_double * 9), ("t_alt", C.c_double * 3), ("err_alt", C.c_double), ("sq_err_sum_alt", C.c_double)]


BUNDLE_DEGENERATE = 3
MAX_RIGID_BUNDLE_MEMBERS = 64


class RigCamera(C.Structure):
    """amdAprilTagsRigCamera_t: the rig frame in the camera frame, X_cam = R X_rig + t (R row-major)."""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3)]


class RigSlot(C.Structure):
    """amdAprilTagsRigSlot_t."""
    _fields_ = [("group", C.c_uint32), ("camera", C.c_uint32)]


class RigBundlePose(C.Structure):
    """amdAprilTagsRigBundlePose_t."""
    _fields_ = [("group", C.c_uint32), ("bundle", C.c_uint32), ("status", C.c_uint32), ("nobs", C.c_uint32), ("nskipped", C.c_uint32),
                ("ndropped", C.c_uint32), ("ncams", C.c_uint32), ("seed_frame", C.c_uint32), ("seed", C.c_uint32), ("chosen", C.c_uint32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("err", C.c_double), ("sq_err_sum", C.c_double),
                ("R_alt", C.c_double * 9), ("t_alt", C.c_double * 3), ("err_alt", C.c_double), ("sq_err_sum_alt", C.c_double)]


RIG_NO_CAMERA = 0xFFFFFFFF
MAX_RIG_CAMERAS, MAX_RIG_OBSERVATIONS = 16, 64


def rig_cameras(cams):
    """[(R (3 x 3), t (3))] as an array of RigCamera; None for an empty list."""
    cams = list(cams or [])
    if not cams:
        return None
    arr = (RigCamera * len(cams))()
    for i, (R, t) in enumerate(cams):
        arr[i].R = (C.c_double * 9)(*[float(v) for v in np.asarray(R, dtype=np.float64).reshape(-1)])
        arr[i].t = (C.c_double * 3)(*[float(v) for v in np.asarray(t, dtype=np.float64).reshape(-1)])
    return arr


class RefinedPose(C.Structure):
    """amdAprilTagsRefinedPose_t."""
    _fields_ = [("status", C.c_uint32), ("chosen", C.c_uint32), ("R", C.c_double * 9), ("t", C.c_double * 3), ("err", C.c_double),
                ("R_alt", C.c_double * 9), ("t_alt", C.c_double * 3), ("err_alt", C.c_double), ("err_homography", C.c_double)]


POSE_REFINED, POSE_REFINED_NO_ALT, POSE_DEGENERATE = 0, 1, 2
MAX_POSE_ITERATIONS = 200


class PoseCovariance(C.Structure):
    """amdAprilTagsPoseCovariance_t."""
    _fields_ = [("cov", C.c_double * 36), ("cov_alt", C.c_double * 36), ("sq_err_sum", C.c_double), ("sq_err_sum_alt", C.c_double),
                ("valid", C.c_uint32), ("reserved", C.c_uint32)]


# the same record as a numpy dtype: what detector.refined_pose_covariances / bundle_pose_covariances_ex hand out
POSE_COV_DTYPE = np.dtype([("cov", "<f8", (6, 6)), ("cov_alt", "<f8", (6, 6)), ("sq_err_sum", "<f8"), ("sq_err_sum_alt", "<f8"),
                           ("valid", "<u4"), ("reserved", "<u4")])
assert POSE_COV_DTYPE.itemsize == C.sizeof(PoseCovariance)


class UndistortedDetection(C.Structure):
    """amdAprilTagsUndistortedDetection_t."""
    _fields_ = [("status", C.c_uint32), ("reserved", C.c_uint32), ("H", C.c_double * 9), ("c", C.c_double * 2), ("p", (C.c_double * 2) * 4),
                ("R", C.c_double * 9), ("t", C.c_double * 3)]


# the same record as a numpy dtype (detector.debug_undistort)
UNDISTORTED_DTYPE = np.dtype([("status", "<u4"), ("reserved", "<u4"), ("H", "<f8", (9,)), ("c", "<f8", (2,)), ("p", "<f8", (4, 2)),
                              ("R", "<f8", (9,)), ("t", "<f8", (3,))])
assert UNDISTORTED_DTYPE.itemsize == C.sizeof(UndistortedDetection)
UNDISTORT_OK, UNDISTORT_INVALID = 0, 1
UNDISTORT_ITERATIONS = 20


class TagEntry(C.Structure):
    """amdAprilTagsTagEntry_t."""
    _fields_ = [("family_index", C.c_uint32), ("id", C.c_uint32), ("size", C.c_float), ("reserved", C.c_uint32)]


MAX_TAG_ENTRIES = 4096
TAG_ID_ANY = 0xFFFF


def tag_entries(tags, families):
    """The amdAprilTagsTagEntry_t array of tags = [(family, id, size)] for a handle of `families` (names): family is a name of that
    list or an index into it; id an int, "*" (every id of the family without an entry of its own) or an inclusive (first, last)
    range, which becomes one entry per id; size in metres, 0 for the handle's tag_size.  None for an empty list."""
    rows = []
    for fam, tid, size in (tags or []):
        fi = families.index(fam) if isinstance(fam, str) else int(fam)
        if isinstance(tid, str):
            if tid != "*":
                raise ValueError("tag id %r: an int, \"*\" or (first, last)" % (tid,))
            ids = [TAG_ID_ANY]
        elif isinstance(tid, (tuple, list)):
            ids = list(range(int(tid[0]), int(tid[1]) + 1))
        else:
            ids = [int(tid)]
        rows += [(fi, i, float(size)) for i in ids]
    if not rows:
        return None
    arr = (TagEntry * len(rows))()
    for e, (fi, i, size) in zip(arr, rows):
        e.family_index, e.id, e.size, e.reserved = fi, i, size, 0
    return arr


class Float2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class TagID(C.Structure):
    _fields_ = [("id", C.c_uint16), ("corners", Float2 * 4), ("hamming_error", C.c_uint16),
                ("orientation", C.c_float * 9), ("translation", C.c_float * 3), ("family", C.c_uint16),
                ("reserved", C.c_uint16), ("decision_margin", C.c_float), ("center", Float2)]


class DetectionEx(C.Structure):
    _fields_ = [("family", C.c_int32), ("id", C.c_int32), ("hamming", C.c_int32), ("decision_margin", C.c_float),
                ("H", C.c_double * 9), ("c", C.c_double * 2), ("p", (C.c_double * 2) * 4), ("R", C.c_double * 9),
                ("t", C.c_double * 3)]


assert DET_DTYPE.itemsize == C.sizeof(DetectionEx)


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("tile_size", C.c_uint32), ("decimate", C.c_uint32),
                ("num_families", C.c_uint32), ("families", C.c_int * 4), ("intrinsics", Intrinsics),
                ("tag_size", C.c_float), ("max_batch", C.c_uint32), ("refine_edges", C.c_uint32),
                ("max_hamming", C.c_uint32), ("decode_sharpening", C.c_float), ("max_points", C.c_uint32),
                ("hash_slots", C.c_uint32), ("max_clusters", C.c_uint32), ("max_quads", C.c_uint32),
                ("max_detections", C.c_uint32), ("device", C.c_int32), ("skew", C.c_float), ("corner_convention", C.c_uint32),
                ("no_graph_replay", C.c_uint32), ("no_stream_priorities", C.c_uint32)]


# every symbol include/apriltag_amd.h declares
EXPORTS = ["amdAprilTagsDefaultConfig", "amdCreateAprilTagsDetector", "amdCreateAprilTagsDetectorEx",
           "amdAprilTagsDestroy", "amdAprilTagsDetect", "amdAprilTagsDetectBatch", "amdAprilTagsDetectBatchEx",
           "amdAprilTagsSubmitBatch", "amdAprilTagsWaitBatch", "amdAprilTagsWaitBatchEx", "amdAprilTagsSetFrameSkews",
           "amdAprilTagsGetFrameFlags", "amdAprilTagsConvertToMono8", "amdAprilTagsRegisterFamily",
           "amdAprilTagsRegisterFamilyEx", "amdAprilTagsUnregisterFamily",
           "amdAprilTagsFamilyInfo", "amdAprilTagsFamilyFromName", "amdAprilTagsStageName",
           "amdAprilTagsSetProfiling", "amdAprilTagsGetStageMs", "amdAprilTagsThresholdOnly",
           "amdAprilTagsDebugCopy", "amdAprilTagsDebugMath", "amdAprilTagsDeviceAlloc", "amdAprilTagsDeviceFree",
           "amdAprilTagsCopyToDevice", "amdAprilTagsResizeMono8", "amdAprilTagsRectifyMono8",
           "amdAprilTagsGetDeviceBytes", "amdAprilTagsDebugSetSubmissionPath", "amdAprilTagsDebugLastSubmissionPath", "amdAprilTagsDebugLateWaits",
           "amdAprilTagsEncodingFromName", "amdAprilTagsDetectColor", "amdAprilTagsDetectBatchColor", "amdAprilTagsDetectBatchColorEx",
           "amdAprilTagsSubmitBatchColor", "amdAprilTagsThresholdOnlyColor", "amdAprilTagsCopyToDeviceAsync", "amdAprilTagsStreamCreate",
           "amdAprilTagsStreamDestroy", "amdAprilTagsDebugGraphReplay", "amdAprilTagsConfigLayoutVersion",
           "amdAprilTagsSetQuadSigma", "amdAprilTagsDebugQuadSigmaTaps", "amdAprilTagsSetPerFrameSizes",
           "amdAprilTagsSetRectification", "amdAprilTagsSetResize", "amdAprilTagsDistortionFromName",
           "amdAprilTagsSetRectificationEx", "amdAprilTagsRectifyMono8Ex", "amdAprilTagsSetBundles", "amdAprilTagsGetBundlePoses",
           "amdAprilTagsDebugLastGraphNodes", "amdAprilTagsSetPoseRefinement", "amdAprilTagsGetRefinedPoses",
           "amdAprilTagsSetBundlesEx", "amdAprilTagsGetBundlePosesEx", "amdAprilTagsDebugReconcile",
           "amdAprilTagsSetPoseCovariance", "amdAprilTagsGetRefinedPoseCovariances", "amdAprilTagsGetBundlePoseCovariancesEx",
           "amdAprilTagsSetCornerUndistortion", "amdAprilTagsGetUndistortedDetections", "amdAprilTagsDebugUndistort",
           "amdAprilTagsSetRig", "amdAprilTagsSetRigSlots", "amdAprilTagsGetRigBundlePoses",
           "amdAprilTagsConvertRawToMono8", "amdAprilTagsSetRawShift", "amdAprilTagsSetTagTable"]
PATH_AUTO, PATH_LATENCY, PATH_THROUGHPUT = 0, 1, 2
ENCODINGS = {"mono8": 0, "rgb8": 1, "bgr8": 2, "rgba8": 3, "bgra8": 4,   # amdAprilTagsEncoding
             "bayer_rggb8": 5, "bayer_bggr8": 6, "bayer_gbrg8": 7, "bayer_grbg8": 8, "mono16": 9,
             "bayer_rggb16": 10, "bayer_bggr16": 11, "bayer_gbrg16": 12, "bayer_grbg16": 13}
RAW_ENCODINGS = tuple(n for n, v in ENCODINGS.items() if v >= 5)   # one sample per pixel: Bayer patterns and mono16
DISTORTIONS = {"plumb_bob": 0, "rational_polynomial": 1, "equidistant": 2}   # amdAprilTagsDistortion
DISTORTION_COEFFS = {"plumb_bob": 5, "rational_polynomial": 8, "equidistant": 4}
ENC_CHANNELS = {"mono8": 1, "rgb8": 3, "bgr8": 3, "rgba8": 4, "bgra8": 4}
ENC_CHANNELS.update({n: 1 for n in RAW_ENCODINGS})
ENC_SAMPLE_BYTES = {n: (2 if n.endswith("16") else 1) for n in ENCODINGS}

_lib = None


def lib():
    """Loads libapriltag_amd.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libapriltag_amd.so is missing: run `python -m isaac_ros_apriltag_amd.build` "
                           "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    H = C.c_void_p
    L.amdAprilTagsDefaultConfig.argtypes = [C.POINTER(Config), C.c_uint32, C.c_uint32]
    L.amdAprilTagsDefaultConfig.restype = None
    L.amdCreateAprilTagsDetector.argtypes = [C.POINTER(H), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                             C.POINTER(Intrinsics), C.c_float]
    L.amdCreateAprilTagsDetectorEx.argtypes = [C.POINTER(H), C.POINTER(Config)]
    L.amdAprilTagsDestroy.argtypes = [H]
    L.amdAprilTagsDetect.argtypes = [H, C.POINTER(ImageInput), C.POINTER(TagID), C.POINTER(C.c_uint32), C.c_uint32, H]
    L.amdAprilTagsDetectBatch.argtypes = [H, C.c_uint32, C.POINTER(ImageInput), C.POINTER(Intrinsics),
                                          C.POINTER(TagID), C.POINTER(C.c_uint32), C.c_uint32, H]
    L.amdAprilTagsDetectBatchEx.argtypes = [H, C.c_uint32, C.POINTER(ImageInput), C.POINTER(Intrinsics),
                                            C.POINTER(DetectionEx), C.POINTER(C.c_uint32), C.c_uint32, H]
    L.amdAprilTagsSubmitBatch.argtypes = [H, C.c_uint32, C.POINTER(ImageInput), C.POINTER(Intrinsics), C.c_uint32, H]
    L.amdAprilTagsEncodingFromName.argtypes = [C.c_char_p]
    L.amdAprilTagsDetectColor.argtypes = [H, C.POINTER(ImageInput), C.c_int, C.POINTER(TagID), C.POINTER(C.c_uint32), C.c_uint32, H]
    L.amdAprilTagsDetectBatchColor.argtypes = [H, C.c_uint32, C.POINTER(ImageInput), C.c_int, C.POINTER(Intrinsics),
                                               C.POINTER(TagID), C.POINTER(C.c_uint32), C.c_uint32, H]
    L.amdAprilTagsDetectBatchColorEx.argtypes = [H, C.c_uint32, C.POINTER(ImageInput), C.c_int, C.POINTER(Intrinsics),
                                                 C.POINTER(DetectionEx), C.POINTER(C.c_uint32), C.c_uint32, H]
    L.amdAprilTagsSubmitBatchColor.argtypes = [H, C.c_uint32, C.POINTER(ImageInput), C.c_int, C.POINTER(Intrinsics), C.c_uint32, H]
    L.amdAprilTagsThresholdOnlyColor.argtypes = [H, C.c_uint32, C.POINTER(ImageInput), C.c_int, H]
    L.amdAprilTagsWaitBatch.argtypes = [H, C.POINTER(TagID), C.POINTER(C.c_uint32)]
    L.amdAprilTagsWaitBatchEx.argtypes = [H, C.POINTER(DetectionEx), C.POINTER(C.c_uint32)]
    L.amdAprilTagsSetFrameSkews.argtypes = [H, C.c_uint32, C.POINTER(C.c_float)]
    L.amdAprilTagsGetFrameFlags.argtypes = [H, C.POINTER(C.c_uint32), C.c_uint32]
    L.amdAprilTagsConvertToMono8.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                             C.c_size_t, H]
    L.amdAprilTagsRegisterFamily.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32]
    L.amdAprilTagsRegisterFamilyEx.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.POINTER(C.c_int8), C.POINTER(C.c_int8), C.c_uint32,
                                               C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.c_uint32]
    L.amdAprilTagsFamilyInfo.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint64))]
    L.amdAprilTagsUnregisterFamily.argtypes = [C.c_int]
    L.amdAprilTagsFamilyFromName.argtypes = [C.c_char_p]
    L.amdAprilTagsStageName.argtypes = [C.c_uint32]
    L.amdAprilTagsStageName.restype = C.c_char_p
    L.amdAprilTagsSetProfiling.argtypes = [H, C.c_int]
    L.amdAprilTagsGetStageMs.argtypes = [H, C.POINTER(C.c_float)]
    L.amdAprilTagsThresholdOnly.argtypes = [H, C.c_uint32, C.POINTER(ImageInput), H]
    L.amdAprilTagsDebugCopy.argtypes = [H, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.amdAprilTagsDeviceAlloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.amdAprilTagsDeviceFree.argtypes = [C.c_void_p]
    L.amdAprilTagsCopyToDevice.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, H]
    L.amdAprilTagsCopyToDeviceAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, H]
    L.amdAprilTagsStreamCreate.argtypes = [C.POINTER(H)]
    L.amdAprilTagsStreamDestroy.argtypes = [H]
    L.amdAprilTagsResizeMono8.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32,
                                          C.c_uint32, H]
    L.amdAprilTagsRectifyMono8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                           C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), H]
    L.amdAprilTagsGetDeviceBytes.argtypes = [H, C.POINTER(C.c_size_t)]
    L.amdAprilTagsDebugSetSubmissionPath.argtypes = [H, C.c_int]
    L.amdAprilTagsDebugLastSubmissionPath.argtypes = [H]
    L.amdAprilTagsDebugLateWaits.argtypes = [H]
    L.amdAprilTagsDebugGraphReplay.argtypes = [H, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.amdAprilTagsDebugMath.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.amdAprilTagsSetQuadSigma.argtypes = [H, C.c_float]
    L.amdAprilTagsSetPerFrameSizes.argtypes = [H, C.c_int]
    L.amdAprilTagsSetRectification.argtypes = [H, C.c_uint32, C.POINTER(CameraModel)]
    L.amdAprilTagsSetResize.argtypes = [H, C.c_uint32, C.POINTER(Size)]
    L.amdAprilTagsDistortionFromName.argtypes = [C.c_char_p]
    L.amdAprilTagsSetRectificationEx.argtypes = [H, C.c_uint32, C.POINTER(CameraModelEx)]
    L.amdAprilTagsRectifyMono8Ex.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                             C.POINTER(CameraModelEx), H]
    L.amdAprilTagsDebugLastGraphNodes.argtypes = [H]
    L.amdAprilTagsSetBundles.argtypes = [H, C.c_uint32, C.POINTER(Bundle)]
    L.amdAprilTagsGetBundlePoses.argtypes = [H, C.POINTER(BundlePose), C.c_uint32]
    L.amdAprilTagsSetBundlesEx.argtypes = [H, C.c_uint32, C.POINTER(BundleEx)]
    L.amdAprilTagsGetBundlePosesEx.argtypes = [H, C.POINTER(BundlePoseEx), C.c_uint32]
    L.amdAprilTagsSetPoseRefinement.argtypes = [H, C.c_uint32]
    L.amdAprilTagsGetRefinedPoses.argtypes = [H, C.c_uint32, C.POINTER(RefinedPose), C.c_uint32, C.POINTER(C.c_uint32)]
    L.amdAprilTagsSetPoseCovariance.argtypes = [H, C.c_double]
    L.amdAprilTagsGetRefinedPoseCovariances.argtypes = [H, C.c_uint32, C.POINTER(PoseCovariance), C.c_uint32, C.POINTER(C.c_uint32)]
    L.amdAprilTagsGetBundlePoseCovariancesEx.argtypes = [H, C.POINTER(PoseCovariance), C.c_uint32]
    L.amdAprilTagsDebugReconcile.argtypes = [H, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.amdAprilTagsSetCornerUndistortion.argtypes = [H, C.c_uint32, C.POINTER(CameraModelEx)]
    L.amdAprilTagsGetUndistortedDetections.argtypes = [H, C.c_uint32, C.POINTER(UndistortedDetection), C.c_uint32, C.POINTER(C.c_uint32)]
    L.amdAprilTagsDebugUndistort.argtypes = [H, C.c_uint32, C.c_void_p, C.POINTER(CameraModelEx), C.c_void_p, C.c_void_p]
    L.amdAprilTagsSetRig.argtypes = [H, C.c_uint32, C.POINTER(RigCamera)]
    L.amdAprilTagsSetRigSlots.argtypes = [H, C.c_uint32, C.POINTER(RigSlot)]
    L.amdAprilTagsGetRigBundlePoses.argtypes = [H, C.POINTER(RigBundlePose), C.c_uint32]
    L.amdAprilTagsConvertRawToMono8.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, H]
    L.amdAprilTagsSetRawShift.argtypes = [H, C.c_uint32]
    L.amdAprilTagsSetTagTable.argtypes = [H, C.c_uint32, C.POINTER(TagEntry), C.c_uint32]
    L.amdAprilTagsDebugQuadSigmaTaps.argtypes =[C.c_float, C.POINTER(C.c_uint8), C.c_uint32, C.POINTER(C.c_uint32)]
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is C.c_int or name in ("amdAprilTagsFamilyFromName", "amdAprilTagsEncodingFromName", "amdAprilTagsDistortionFromName"):
            fn.restype = C.c_int
    _lib = L
    return L


class AprilTagsError(RuntimeError):
    def __init__(self, where, code):
        super().__init__("%s failed: %s (error code %d)" % (where, STATUS.get(code, "?"), code))
        self.code = code


def _check(where, rc):
    if rc != 0:
        raise AprilTagsError(where, rc)


def stage_names():
    return [lib().amdAprilTagsStageName(i).decode() for i in range(NUM_STAGES)]


def family_info(name_or_enum):
    L = lib()
    fam = name_or_enum if isinstance(name_or_enum, int) else L.amdAprilTagsFamilyFromName(name_or_enum.encode())
    if fam < 0:
        raise ValueError("unknown family %r" % (name_or_enum,))
    nm, d, n, codes = C.c_char_p(), C.c_uint32(), C.c_uint32(), C.POINTER(C.c_uint64)()
    _check("amdAprilTagsFamilyInfo", L.amdAprilTagsFamilyInfo(fam, C.byref(nm), C.byref(d), C.byref(n), C.byref(codes)))
    return {"enum": fam, "name": nm.value.decode(), "d": d.value, "codes": [int(codes[i]) for i in range(n.value)]}


def register_family(slot, name, d, codes):
    """Classic d x d family (row-major codes) in a registrable slot."""
    cc = (C.c_uint64 * len(codes))(*[int(c) for c in codes])
    _check("amdAprilTagsRegisterFamily", lib().amdAprilTagsRegisterFamily(slot, name.encode(), d, cc, len(codes)))


def register_family_ex(slot, name, bit_x, bit_y, width_at_border, total_width, reversed_border, codes):
    """AprilTag-3 style layout (bit i at cell (bit_x[i], bit_y[i]) in border coordinates)."""
    n = len(bit_x)
    bx = (C.c_int8 * n)(*[int(v) for v in bit_x])
    by = (C.c_int8 * n)(*[int(v) for v in bit_y])
    cc = (C.c_uint64 * len(codes))(*[int(c) for c in codes])
    _check("amdAprilTagsRegisterFamilyEx", lib().amdAprilTagsRegisterFamilyEx(slot, name.encode(), n, bx, by, width_at_border, total_width,
                                                                             int(bool(reversed_border)), cc, len(codes)))


def unregister_family(slot):
    _check("amdAprilTagsUnregisterFamily", lib().amdAprilTagsUnregisterFamily(slot))


def debug_math(op, a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    out = np.empty_like(a)
    _check("amdAprilTagsDebugMath", lib().amdAprilTagsDebugMath(op, a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data))
    return out


def camera_models(models):
    """[(K, D, Knew)] -> a ctypes array of amdAprilTagsCameraModel_t (None for an empty list).  K, Knew: 3x3 or 9 values; D: up to five
    plumb_bob coefficients, zero-padded."""
    models = list(models or [])
    if not models:
        return None
    arr = (CameraModel * len(models))()
    for m, (K, D, Knew) in zip(arr, models):
        k, d, kn = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (K, D, Knew))
        if k.size != 9 or kn.size != 9 or d.size > 5:
            raise ValueError("a camera model is (K[3x3], D[<= 5], Knew[3x3])")
        m.K[:], m.Knew[:] = list(k), list(kn)
        m.D[:] = list(d) + [0.0] * (5 - d.size)
    return arr


def camera_model_ex(K, D, Knew, model_name="plumb_bob", R=None):
    """One amdAprilTagsCameraModelEx_t.  model_name: a key of DISTORTIONS, or the enum's integer (passed on as it stands, for the
    library to judge); D: up to the kind's coefficients (eight for an integer kind), zero-padded; R: 3x3 or 9 values, None: the
    identity."""
    m = CameraModelEx()
    if isinstance(model_name, str):
        if model_name not in DISTORTIONS:
            raise ValueError("unknown distortion model %r: known are plumb_bob, rational_polynomial and equidistant" % (model_name,))
        m.kind, nmax = DISTORTIONS[model_name], DISTORTION_COEFFS[model_name]
    else:
        m.kind, nmax = int(model_name), 8
    k, d, kn = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (K, D, Knew))
    r = np.eye(3).reshape(-1) if R is None else np.asarray(R, dtype=np.float64).reshape(-1)
    if k.size != 9 or kn.size != 9 or r.size != 9 or d.size > nmax:
        raise ValueError("a camera model is (K[3x3], D[<= %d for this kind], Knew[3x3], model_name, R[3x3] or None)" % nmax)
    m.K[:], m.Knew[:], m.R[:] = list(k), list(kn), list(r)
    m.D[:] = list(d) + [0.0] * (8 - d.size)
    return m


def camera_models_ex(models):
    """[(K, D, Knew) or (K, D, Knew, model_name, R)] -> a ctypes array of amdAprilTagsCameraModelEx_t (a 3-tuple: plumb_bob, R = I)."""
    models = list(models)
    arr = (CameraModelEx * len(models))()
    for i, m in enumerate(models):
        if len(m) not in (3, 5):
            raise ValueError("a camera model is (K, D, Knew) or (K, D, Knew, model_name, R)")
        arr[i] = camera_model_ex(*m)
    return arr


def sizes(pairs):
    """[(width, height)] -> a ctypes array of amdAprilTagsSize_t (None for an empty list)."""
    pairs = list(pairs or [])
    if not pairs:
        return None
    arr = (Size * len(pairs))()
    for s, (w, h) in zip(arr, pairs):
        s.width, s.height = int(w), int(h)
    return arr


def bundles(specs):
    """[{"name", "members": [(family_index, id, x, y, size)], "max_hamming" (2), "min_decision_margin" (0.0), "min_tags" (1)}] -> a ctypes
    array of amdAprilTagsBundle_t (None for an empty list); the member arrays it points into are kept alive on the array."""
    specs = list(specs or [])
    if not specs:
        return None
    arr = (Bundle * len(specs))()
    keep = []
    for b, spec in zip(arr, specs):
        mem = list(spec["members"])
        m = (BundleMember * max(len(mem), 1))()
        for dst, (fam, tid, x, y, size) in zip(m, mem):
            dst.family_index, dst.id, dst.x, dst.y, dst.size = int(fam), int(tid), float(x), float(y), float(size)
        keep.append(m)
        b.members, b.nmembers = C.cast(m, C.POINTER(BundleMember)), len(mem)
        b.max_hamming = int(spec.get("max_hamming", 2))
        b.min_decision_margin = float(spec.get("min_decision_margin", 0.0))
        b.min_tags = int(spec.get("min_tags", 1))
        name = spec.get("name", "").encode()
        if len(name) > 31:
            raise ValueError("a bundle name has at most 31 characters")
        b.name = name
    arr._keep = keep
    return arr


def bundles_ex(specs):
    """[{"name", "iterations" (50), "members": [(family_index, id, R (3 x 3), t (3), size)], "max_hamming" (2), "min_decision_margin"
    (0.0), "min_tags" (1)}] -> a ctypes array of amdAprilTagsBundleEx_t (None for an empty list); the member arrays it points into are
    kept alive on the array."""
    specs = list(specs or [])
    if not specs:
        return None
    arr = (BundleEx * len(specs))()
    keep = []
    for b, spec in zip(arr, specs):
        mem = list(spec["members"])
        m = (BundleMemberEx * max(len(mem), 1))()
        for dst, (fam, tid, R, t, size) in zip(m, mem):
            dst.family_index, dst.id, dst.size = int(fam), int(tid), float(size)
            dst.R = (C.c_double * 9)(*[float(v) for v in np.asarray(R, dtype=np.float64).reshape(-1)])
            dst.t = (C.c_double * 3)(*[float(v) for v in np.asarray(t, dtype=np.float64).reshape(-1)])
        keep.append(m)
        b.members, b.nmembers = C.cast(m, C.POINTER(BundleMemberEx)), len(mem)
        b.max_hamming = int(spec.get("max_hamming", 2))
        b.min_decision_margin = float(spec.get("min_decision_margin", 0.0))
        b.min_tags = int(spec.get("min_tags", 1))
        b.iterations = int(spec.get("iterations", 50))
        name = spec.get("name", "").encode()
        if len(name) > 31:
            raise ValueError("a bundle name has at most 31 characters")
        b.name = name
    arr._keep = keep
    return arr


def quad_sigma_taps(sigma):
    """amdAprilTagsDebugQuadSigmaTaps: upstream's taps for quad_sigma (an empty list for the identity)."""
    taps = (C.c_uint8 * 17)()
    ksz = C.c_uint32()
    _check("amdAprilTagsDebugQuadSigmaTaps", lib().amdAprilTagsDebugQuadSigmaTaps(float(sigma), taps, 17, C.byref(ksz)))
    return [int(taps[i]) for i in range(ksz.value)] if ksz.value > 1 else []
