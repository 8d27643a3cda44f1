"""ctypes view of libapriltag_node.so -- the ROS-free C++ mirror of the reference node shell
(include/apriltag_node_shell.hpp).  Used by the tests to drive the node logic the way the reference's
gtest / launch tests drive AprilTagNode."""
import ctypes as C
import os

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))


class ShellDetection(C.Structure):
    _fields_ = [("id", C.c_int32), ("family", C.c_char * 32), ("center", C.c_double * 2),
                ("corners", (C.c_double * 2) * 4), ("position", C.c_double * 3),
                ("orientation_xyzw", C.c_double * 4), ("child_frame_id", C.c_char * 48)]


class ShellBundle(C.Structure):
    """NodeOptions::bundles through the flat view: members holds four doubles per member -- id, x, y, size."""
    _fields_ = [("name", C.c_char * 32), ("members", C.POINTER(C.c_double)), ("nmembers", C.c_uint32), ("max_hamming", C.c_uint32),
                ("min_tags", C.c_uint32), ("pad", C.c_uint32), ("min_decision_margin", C.c_double)]


class ShellTag(C.Structure):
    """NodeOptions::tags through the flat view: one tag's id, size (0: the node's) and TF child frame ("": "family:id")."""
    _fields_ = [("id", C.c_uint32), ("size", C.c_double), ("frame", C.c_char * 64)]


def _shell_tags(tags):
    """tags: [(id, size, frame)] or [{"id", "size", "frame"}] -> the flat view's array."""
    arr = (ShellTag * max(len(tags), 1))()
    for e, t in zip(arr, tags):
        tid, size, frame = (t["id"], t.get("size", 0.0), t.get("frame", "")) if isinstance(t, dict) else t
        name = (frame or "").encode()
        if len(name) > 63:
            raise ValueError("tags: frame %r is longer than 47 characters" % (frame,))
        e.id, e.size, e.frame = int(tid), float(size), name
    return arr


class ShellRigidBundle(C.Structure):
    """NodeOptions::rigid_bundles through the flat view: members holds nine doubles per member -- id, x, y, z, qw, qx, qy, qz, size."""
    _fields_ = [("name", C.c_char * 32), ("members", C.POINTER(C.c_double)), ("nmembers", C.c_uint32), ("max_hamming", C.c_uint32),
                ("min_tags", C.c_uint32), ("iterations", C.c_uint32), ("min_decision_margin", C.c_double)]


class ShellRigidBundlePose(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("status", C.c_uint32), ("ntags", C.c_uint32), ("nskipped", C.c_uint32), ("seed", C.c_uint32),
                ("chosen", C.c_uint32), ("pad", C.c_uint32), ("R", C.c_double * 9), ("t", C.c_double * 3), ("err", C.c_double),
                ("sq_err_sum", C.c_double), ("R_alt", C.c_double * 9), ("t_alt", C.c_double * 3), ("err_alt", C.c_double),
                ("sq_err_sum_alt", C.c_double)]


class ShellTransform(C.Structure):
    _fields_ = [("child_frame_id", C.c_char * 48), ("frame_id", C.c_char * 48), ("sec", C.c_int32), ("nanosec", C.c_uint32),
                ("translation", C.c_double * 3), ("rotation_xyzw", C.c_double * 4)]


class ShellBundlePose(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("status", C.c_uint32), ("ntags", C.c_uint32), ("nskipped", C.c_uint32), ("pad", C.c_uint32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("sq_err_sum", C.c_double)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = _build.LIB_NODE
        if not os.path.exists(path):
            _build.build_node()
        L = C.CDLL(path)
        L.node_shell_create.restype = C.c_void_p
        L.node_shell_create.argtypes = [C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
        L.node_shell_create_strict.restype = C.c_void_p
        L.node_shell_create_strict.argtypes = L.node_shell_create.argtypes
        L.node_shell_create_ex.restype = C.c_void_p
        L.node_shell_create_ex.argtypes = [C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double,
                                           C.c_char_p, C.c_size_t]
        L.node_shell_create_raw.restype = C.c_void_p
        L.node_shell_create_raw.argtypes = [C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint32,
                                            C.c_char_p, C.c_size_t]
        L.node_shell_set_bigendian.restype = None
        L.node_shell_set_bigendian.argtypes = [C.c_void_p, C.c_int]
        L.node_shell_create_opts.restype = C.c_void_p
        L.node_shell_create_opts.argtypes = [C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_int,
                                             C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]
        L.node_shell_camera_model.restype = C.c_int
        L.node_shell_camera_model.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_char_p, C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), C.c_char_p, C.c_size_t]
        L.node_shell_camera_model_ex.restype = C.c_int
        L.node_shell_camera_model_ex.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_char_p, C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_char_p, C.c_size_t]
        L.node_shell_on_frame_full.restype = C.c_int
        L.node_shell_on_frame_full.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_char_p, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.c_char_p, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32,
                                               C.POINTER(ShellDetection), C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.node_shell_multi_on_frame_full.restype = C.c_int
        L.node_shell_multi_on_frame_full.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32,
                                                     C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_char_p,
                                                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_char_p, C.c_int32, C.c_uint32,
                                                     C.c_int32, C.c_uint32, C.c_char_p, C.c_size_t]
        L.node_shell_destroy.argtypes = [C.c_void_p]
        L.node_shell_on_frame_info.restype = C.c_int
        L.node_shell_on_frame_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_char_p, C.POINTER(C.c_double),
                                               C.c_char_p, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32,
                                               C.POINTER(ShellDetection), C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.node_shell_multi_create_opts.restype = C.c_void_p
        L.node_shell_multi_create_opts.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                   C.c_double, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_char_p,
                                                   C.c_size_t]
        L.node_shell_multi_on_frame_info.restype = C.c_int
        L.node_shell_multi_on_frame_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32,
                                                     C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_char_p,
                                                     C.POINTER(C.c_double), C.c_char_p, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32,
                                                     C.c_char_p, C.c_size_t]
        L.node_shell_on_frame.restype = C.c_int
        L.node_shell_on_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_double), C.c_char_p, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32,
                                          C.POINTER(ShellDetection), C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.node_shell_multi_create.restype = C.c_void_p
        L.node_shell_multi_create.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
        L.node_shell_multi_create_ex.restype = C.c_void_p
        L.node_shell_multi_create_ex.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                 C.c_double, C.c_char_p, C.c_size_t]
        L.node_shell_multi_create_sized.restype = C.c_void_p
        L.node_shell_multi_create_sized.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                    C.c_double, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]
        L.node_shell_multi_destroy.argtypes = [C.c_void_p]
        L.node_shell_multi_on_frame.restype = C.c_int
        L.node_shell_multi_on_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.POINTER(C.c_double), C.c_char_p, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32, C.c_char_p, C.c_size_t]
        L.node_shell_multi_flush.restype = C.c_int
        L.node_shell_multi_flush.argtypes = [C.c_void_p]
        L.node_shell_multi_publishes.restype = C.c_int
        L.node_shell_multi_publishes.argtypes = [C.c_void_p, C.c_int]
        L.node_shell_multi_last.restype = C.c_int
        L.node_shell_multi_last.argtypes = [C.c_void_p, C.c_int, C.POINTER(ShellDetection), C.c_int, C.c_char_p, C.c_size_t,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
        L.node_shell_create_bundles.restype = C.c_void_p
        L.node_shell_create_bundles.argtypes = [C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                C.POINTER(ShellBundle), C.c_char_p, C.c_size_t]
        L.node_shell_multi_create_bundles.restype = C.c_void_p
        L.node_shell_multi_create_bundles.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                      C.c_int, C.POINTER(ShellBundle), C.c_char_p, C.c_size_t]
        L.node_shell_create_refined.restype = C.c_void_p
        L.node_shell_create_refined.argtypes = [C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_char_p, C.c_size_t]
        L.node_shell_create_tags.restype = C.c_void_p
        L.node_shell_create_tags.argtypes = [C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_int, C.POINTER(ShellTag),
                                             C.c_int, C.c_char_p, C.c_size_t]
        L.node_shell_multi_create_tags.restype = C.c_void_p
        L.node_shell_multi_create_tags.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint32,
                                                   C.c_int, C.POINTER(ShellTag), C.c_int, C.c_char_p, C.c_size_t]
        L.node_shell_multi_create_refined.restype = C.c_void_p
        L.node_shell_multi_create_refined.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint32,
                                                      C.c_char_p, C.c_size_t]
        L.node_shell_create_undistort_refined.restype = C.c_void_p
        L.node_shell_create_undistort_refined.argtypes = [C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_double,
                                                          C.c_char_p, C.c_size_t]
        L.node_shell_multi_create_undistort_refined.restype = C.c_void_p
        L.node_shell_multi_create_undistort_refined.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                                C.c_uint32, C.c_char_p, C.c_size_t]
        L.node_shell_last_transforms.restype = C.c_int
        L.node_shell_last_transforms.argtypes = [C.c_void_p, C.POINTER(ShellTransform), C.c_int]
        L.node_shell_last_bundle_poses.restype = C.c_int
        L.node_shell_last_bundle_poses.argtypes = [C.c_void_p, C.POINTER(ShellBundlePose), C.c_int]
        L.node_shell_multi_last_transforms.restype = C.c_int
        L.node_shell_multi_last_transforms.argtypes = [C.c_void_p, C.c_int, C.POINTER(ShellTransform), C.c_int]
        L.node_shell_multi_last_bundle_poses.restype = C.c_int
        L.node_shell_multi_last_bundle_poses.argtypes = [C.c_void_p, C.c_int, C.POINTER(ShellBundlePose), C.c_int]
        L.node_shell_create_rigid_bundles.restype = C.c_void_p
        L.node_shell_create_rigid_bundles.argtypes = [C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                      C.POINTER(ShellRigidBundle), C.c_char_p, C.c_size_t]
        L.node_shell_multi_create_rigid_bundles.restype = C.c_void_p
        L.node_shell_multi_create_rigid_bundles.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                            C.c_int, C.POINTER(ShellRigidBundle), C.c_char_p, C.c_size_t]
        L.node_shell_last_rigid_bundle_poses.restype = C.c_int
        L.node_shell_last_rigid_bundle_poses.argtypes = [C.c_void_p, C.POINTER(ShellRigidBundlePose), C.c_int]
        L.node_shell_multi_last_rigid_bundle_poses.restype = C.c_int
        L.node_shell_multi_last_rigid_bundle_poses.argtypes = [C.c_void_p, C.c_int, C.POINTER(ShellRigidBundlePose), C.c_int]
        L.node_shell_create_covariance.restype = C.c_void_p
        L.node_shell_create_covariance.argtypes = [C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_int,
                                                   C.POINTER(ShellRigidBundle), C.c_double, C.c_char_p, C.c_size_t]
        L.node_shell_multi_create_covariance.restype = C.c_void_p
        L.node_shell_multi_create_covariance.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                                         C.c_uint32, C.c_int, C.POINTER(ShellRigidBundle), C.c_double, C.c_char_p, C.c_size_t]
        for fn in (L.node_shell_last_covariances, L.node_shell_last_rigid_covariances):
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        for fn in (L.node_shell_multi_last_covariances, L.node_shell_multi_last_rigid_covariances):
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int]
        _lib = L
    return _lib


def _covariances(call, max_out):
    """The 6 x 6 covariances a flat-view call hands out (36 doubles each), as a list of numpy arrays."""
    import numpy as np
    out = (C.c_double * (36 * max_out))()
    n = min(call(out, max_out), max_out)
    return [np.array(out[36 * i:36 * (i + 1)]).reshape(6, 6) for i in range(n)]


def _shell_bundles(bundles):
    """[{"name", "members": [(id, x, y, size)], "max_hamming", "min_decision_margin", "min_tags"}] -> a ShellBundle array (kept alive
    with its member arrays)."""
    arr = (ShellBundle * len(bundles))()
    keep = []
    for b, spec in zip(arr, bundles):
        flat = [float(v) for m in spec["members"] for v in m]
        mem = (C.c_double * max(len(flat), 1))(*flat)
        keep.append(mem)
        b.name = spec.get("name", "").encode()
        b.members, b.nmembers = C.cast(mem, C.POINTER(C.c_double)), len(spec["members"])
        b.max_hamming, b.min_tags = int(spec.get("max_hamming", 2)), int(spec.get("min_tags", 1))
        b.min_decision_margin = float(spec.get("min_decision_margin", 0.0))
    arr._keep = keep
    return arr


def _shell_rigid_bundles(bundles):
    """[{"name", "iterations", "members": [(id, (x, y, z), (qw, qx, qy, qz), size)], "max_hamming", "min_decision_margin", "min_tags"}] ->
    a ShellRigidBundle array (kept alive with its member arrays)."""
    arr = (ShellRigidBundle * len(bundles))()
    keep = []
    for b, spec in zip(arr, bundles):
        flat = [float(v) for (tid, xyz, q, size) in spec["members"] for v in (tid,) + tuple(xyz) + tuple(q) + (size,)]
        mem = (C.c_double * max(len(flat), 1))(*flat)
        keep.append(mem)
        b.name = spec.get("name", "").encode()
        b.members, b.nmembers = C.cast(mem, C.POINTER(C.c_double)), len(spec["members"])
        b.max_hamming, b.min_tags = int(spec.get("max_hamming", 2)), int(spec.get("min_tags", 1))
        b.iterations = int(spec.get("iterations", 50))
        b.min_decision_margin = float(spec.get("min_decision_margin", 0.0))
    arr._keep = keep
    return arr


def _unpack_rigid_bundle_poses(out, n):
    return [{"name": p.name.decode(), "status": int(p.status), "ntags": int(p.ntags), "nskipped": int(p.nskipped), "seed": int(p.seed),
             "chosen": int(p.chosen), "R": list(p.R), "t": list(p.t), "err": float(p.err), "sq_err_sum": float(p.sq_err_sum),
             "R_alt": list(p.R_alt), "t_alt": list(p.t_alt), "err_alt": float(p.err_alt), "sq_err_sum_alt": float(p.sq_err_sum_alt)} for p in out[:n]]


class ShellRigBundlePose(C.Structure):
    """NodeShellRigBundlePose: the rig record of one rigid bundle for one round (include/apriltag_node_shell.hpp: RigBundlePose)."""
    _fields_ = [("name", C.c_char * 32), ("status", C.c_uint32), ("nobs", C.c_uint32), ("nskipped", C.c_uint32), ("ndropped", C.c_uint32),
                ("ncams", C.c_uint32), ("seed_stream", C.c_uint32), ("seed", C.c_uint32), ("chosen", C.c_uint32), ("R", C.c_double * 9),
                ("t", C.c_double * 3), ("err", C.c_double), ("sq_err_sum", C.c_double), ("R_alt", C.c_double * 9), ("t_alt", C.c_double * 3),
                ("err_alt", C.c_double), ("sq_err_sum_alt", C.c_double)]


def _unpack_transforms(out, n):
    return [{"child_frame_id": t.child_frame_id.decode(), "frame_id": t.frame_id.decode(), "stamp": (t.sec, t.nanosec),
             "translation": list(t.translation), "rotation_xyzw": list(t.rotation_xyzw)} for t in out[:n]]


def _unpack_bundle_poses(out, n):
    return [{"name": p.name.decode(), "status": int(p.status), "ntags": int(p.ntags), "nskipped": int(p.nskipped), "R": list(p.R),
             "t": list(p.t), "sq_err_sum": float(p.sq_err_sum)} for p in out[:n]]


def _unpack(out, n):
    dets = []
    for i in range(n):
        d = out[i]
        dets.append({"id": d.id, "family": d.family.decode(), "center": list(d.center),
                     "corners": [[d.corners[c][0], d.corners[c][1]] for c in range(4)],
                     "position": list(d.position), "orientation_xyzw": list(d.orientation_xyzw),
                     "child_frame_id": d.child_frame_id.decode()})
    return dets


def _info_extras(D, distortion_model, P12):
    """sensor_msgs/CameraInfo's D, distortion_model and P as the flat view takes them (None: left empty)."""
    d = (C.c_double * len(D))(*[float(v) for v in D]) if D is not None and len(D) else None
    p = (C.c_double * 12)(*[float(v) for v in P12]) if P12 is not None else None
    return d, (len(D) if d is not None else 0), (distortion_model.encode() if distortion_model is not None else None), p


def camera_model(K9, D=None, distortion_model=None, P12=None):
    """RectificationModel (include/apriltag_node_shell.hpp) of a CameraInfo with these fields: (K[9], D[5], Knew[9]) as lists.
    Raises RuntimeError with the shell's text for a model NodeOptions::rectify does not take.  Host only."""
    k = (C.c_double * 9)(*[float(v) for v in K9])
    d, nd, m, p = _info_extras(D, distortion_model, P12)
    out = (C.c_double * 23)()
    err = C.create_string_buffer(1024)
    if lib().node_shell_camera_model(k, d, nd, m, p, out, err, 1024) != 0:
        raise RuntimeError(err.value.decode())
    v = list(out)
    return v[:9], v[9:14], v[14:]


def _rotation(R):
    """sensor_msgs/CameraInfo's R, 3 x 3 or nine values (None: left all zero, as a monocular driver leaves it)."""
    if R is None:
        return None
    flat = [float(v) for row in R for v in row] if len(R) == 3 else [float(v) for v in R]
    return (C.c_double * 9)(*flat)


def _rectify_flag(rectify):
    """NodeOptions::rectify / rectify_full / undistort_corners as the flat view takes them: False 0, True 1, "full" 2, "corners" 3."""
    if rectify == "full":
        return 2
    if rectify == "corners":
        return 3
    if isinstance(rectify, str):
        raise ValueError("rectify is False, True, \"full\" or \"corners\"")
    return 1 if rectify else 0


def camera_model_ex(K9, D=None, distortion_model=None, P12=None, R=None):
    """RectificationModelEx (include/apriltag_node_shell.hpp) of a CameraInfo with these fields: (kind, K[9], D[8], R[9], Knew[9]).
    Raises RuntimeError with the shell's text for a model NodeOptions::rectify_full does not take.  Host only."""
    k = (C.c_double * 9)(*[float(v) for v in K9])
    d, nd, m, p = _info_extras(D, distortion_model, P12)
    out = (C.c_double * 36)()
    err = C.create_string_buffer(1024)
    if lib().node_shell_camera_model_ex(k, d, nd, m, p, _rotation(R), out, err, 1024) != 0:
        raise RuntimeError(err.value.decode())
    v = list(out)
    return int(v[0]), v[1:10], v[10:18], v[18:27], v[27:]


class AprilTagMultiCameraNode:
    """S camera streams on one GPU, one detector submission per round (include/apriltag_node_shell.hpp)."""

    def __init__(self, num_streams, max_tags=64, size=0.22, tile_size=4, tag_family="tag36h11", backends="CUDA", decimate=1,
                 auto_flush=True, quad_sigma=0.0, max_width=0, max_height=0, rectify=False, resize=None, bundles=None, pose_refinement=0,
                 rigid_bundles=None, pose_covariance=0.0, rig_cameras=None, rig_frame_id="rig", tags=None, tags_listed_only=False):
        """tags, tags_listed_only (NodeOptions::tags, with pose_refinement and nothing else): [(id, size, frame)] -- every listed tag's pose
        at its own size (0: the node's) and its transform under `frame` ("": "family:id"); with tags_listed_only the other tags are
        not reported.  rig_cameras (NodeOptions::rig_cameras, with rigid_bundles and nothing else): [(R, t)] per stream, the rig frame in the
        camera frame -- every round is one instant of the rig: one "rig_bundle:<name>" transform per solved bundle under rig_frame_id
        behind the first served stream's transforms, and rig_bundle_poses() hands out the records.
        max_width, max_height (NodeOptions): both set, streams of every size up to that one are batched together (per-frame image
        sizes); 0: one size, the first frame's, and frames of another size are dropped.  rectify (NodeOptions): every stream's frames are
        undistorted inside the submission with the plumb_bob model of its CameraInfo (on_frame: D, distortion_model, P12); "full"
        (NodeOptions::rectify_full): with any of the three distortion models and the rotation R of its CameraInfo; "corners"
        (NodeOptions::undistort_corners): the frames are detected raw and the detections' corners undistorted under that model -- poses
        and transforms are those of the undistorted corners, corners and centre stay the raw frame's.  resize
        (NodeOptions::resize_width, resize_height): (w, h) -- frames of any size are resized to it inside the submission, behind the
        rectification, and the pose is computed with the scaled camera.  bundles (NodeOptions::bundles, alone among the extensions):
        [{"name", "members": [(id, x, y, size)], ...}] -- one "bundle:<name>" transform per solved bundle behind the tags'.
        pose_refinement (NodeOptions::pose_refinement, alone among the extensions): iterations of the orthogonal-iteration pose -- the
        detections' poses and the tags' transforms are the chosen refined pose.  rigid_bundles (NodeOptions::rigid_bundles, alone among
        the extensions): [{"name", "iterations", "members": [(id, (x, y, z), (qw, qx, qy, qz), size)], ...}] -- one "bundle:<name>"
        transform per solved rigid bundle, from the chosen pose.  pose_covariance (NodeOptions::pose_covariance_sigma_px, with
        pose_refinement and / or rigid_bundles): the corner noise in pixels -- covariances(stream) and rigid_bundle_covariances(stream)
        hand out what the node published."""
        rw, rh = (int(resize[0]), int(resize[1])) if resize else (0, 0)
        err = C.create_string_buffer(1024)
        self._L = lib()
        self.max_tags, self.num_streams = max_tags, num_streams
        if tags or tags_listed_only:
            if bundles or quad_sigma or max_width or max_height or rectify or resize or rigid_bundles or pose_covariance or rig_cameras:
                raise ValueError("tags is served alone by this view, or with pose_refinement")
            arr = _shell_tags(list(tags or []))
            self._h = self._L.node_shell_multi_create_tags(num_streams, max_tags, size, tile_size, tag_family.encode(), backends.encode(), decimate,
                                                           1 if auto_flush else 0, int(pose_refinement), len(tags or []), arr,
                                                           1 if tags_listed_only else 0, err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if rig_cameras:
            if bundles or pose_refinement or quad_sigma or max_width or max_height or rectify or resize or pose_covariance:
                raise ValueError("rig_cameras is served with rigid_bundles by this view, and with nothing else")
            arr = _shell_rigid_bundles(rigid_bundles or [])
            flat = [float(v) for (R, t) in rig_cameras for part in (R, t) for row in part for v in (row if hasattr(row, "__iter__") else (row,))]
            if len(flat) != 12 * len(rig_cameras):
                raise ValueError("rig_cameras: every camera is (R of nine entries, t of three)")
            self._L.node_shell_multi_create_rig.restype = C.c_void_p
            self._L.node_shell_multi_create_rig.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int,
                                                            C.POINTER(ShellRigidBundle), C.c_int, C.POINTER(C.c_double), C.c_char_p, C.c_char_p,
                                                            C.c_size_t]
            self._h = self._L.node_shell_multi_create_rig(num_streams, max_tags, size, tile_size, tag_family.encode(), backends.encode(), decimate,
                                                          1 if auto_flush else 0, len(arr), arr, len(rig_cameras), (C.c_double * len(flat))(*flat),
                                                          rig_frame_id.encode(), err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if pose_covariance:
            if bundles or quad_sigma or max_width or max_height or rectify or resize or not (pose_refinement or rigid_bundles):
                raise ValueError("pose_covariance is served with pose_refinement and / or rigid_bundles by this view, and with nothing else")
            arr = _shell_rigid_bundles(rigid_bundles or [])
            self._h = self._L.node_shell_multi_create_covariance(num_streams, max_tags, size, tile_size, tag_family.encode(), backends.encode(),
                                                                 decimate, 1 if auto_flush else 0, int(pose_refinement), len(arr), arr,
                                                                 float(pose_covariance), err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if rigid_bundles:
            if bundles or pose_refinement or quad_sigma or max_width or max_height or rectify or resize:
                raise ValueError("rigid_bundles is served alone by this view: not with bundles, pose_refinement, quad_sigma, max_width / "
                                 "max_height, rectify or resize")
            arr = _shell_rigid_bundles(rigid_bundles)
            self._h = self._L.node_shell_multi_create_rigid_bundles(num_streams, max_tags, size, tile_size, tag_family.encode(),
                                                                    backends.encode(), decimate, 1 if auto_flush else 0, len(arr), arr, err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if pose_refinement and rectify == "corners" and not (bundles or quad_sigma or max_width or max_height or resize or rigid_bundles
                                                             or pose_covariance):
            # (NodeOptions::undistort_corners beside pose_refinement: the one pair of extensions this view serves together)
            self._h = self._L.node_shell_multi_create_undistort_refined(num_streams, max_tags, size, tile_size, tag_family.encode(),
                                                                        backends.encode(), decimate, 1 if auto_flush else 0,
                                                                        int(pose_refinement), err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if pose_refinement:
            if bundles or quad_sigma or max_width or max_height or rectify or resize:
                raise ValueError("pose_refinement is served alone by this view: not with bundles, quad_sigma, max_width / max_height, rectify or resize")
            self._h = self._L.node_shell_multi_create_refined(num_streams, max_tags, size, tile_size, tag_family.encode(), backends.encode(),
                                                              decimate, 1 if auto_flush else 0, int(pose_refinement), err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if bundles:
            arr = _shell_bundles(bundles)
            self._h = self._L.node_shell_multi_create_bundles(num_streams, max_tags, size, tile_size, tag_family.encode(), backends.encode(),
                                                              decimate, 1 if auto_flush else 0, len(arr), arr, err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        self._h = self._L.node_shell_multi_create_opts(num_streams, max_tags, size, tile_size, tag_family.encode(), backends.encode(),
                                                       decimate, 1 if auto_flush else 0, float(quad_sigma), int(max_width),
                                                       int(max_height), _rectify_flag(rectify), rw, rh, err, 1024)
        if not self._h:
            raise RuntimeError(err.value.decode())
        self.max_tags, self.num_streams = max_tags, num_streams

    def close(self):
        if getattr(self, "_h", None):
            self._L.node_shell_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def on_frame(self, stream, data_ptr, is_device, encoding, width, height, step, K9, frame_id="tf_camera", stamp=(1, 0), info_stamp=None,
                 D=None, distortion_model=None, P12=None, R=None):
        info_stamp = stamp if info_stamp is None else info_stamp
        err = C.create_string_buffer(1024)
        k = (C.c_double * 9)(*[float(v) for v in K9])
        d, nd, m, p = _info_extras(D, distortion_model, P12)
        rc = self._L.node_shell_multi_on_frame_full(self._h, stream, data_ptr, 1 if is_device else 0, encoding.encode(), width, height, step,
                                                    k, d, nd, m, p, _rotation(R), frame_id.encode(), stamp[0], stamp[1], info_stamp[0],
                                                    info_stamp[1], err, 1024)
        if rc == -2:
            raise RuntimeError(err.value.decode())
        return rc == 1

    def transforms(self, stream, max_out=128):
        """The transforms of the last frame published for `stream`: the tags', then one per solved bundle."""
        out = (ShellTransform * max_out)()
        return _unpack_transforms(out, min(self._L.node_shell_multi_last_transforms(self._h, stream, out, max_out), max_out))

    def bundle_poses(self, stream, max_out=8):
        out = (ShellBundlePose * max_out)()
        return _unpack_bundle_poses(out, min(self._L.node_shell_multi_last_bundle_poses(self._h, stream, out, max_out), max_out))

    def rigid_bundle_poses(self, stream, max_out=8):
        out = (ShellRigidBundlePose * max_out)()
        return _unpack_rigid_bundle_poses(out, min(self._L.node_shell_multi_last_rigid_bundle_poses(self._h, stream, out, max_out), max_out))

    def covariances(self, stream):
        """detection.pose.pose.covariance of the last message published for `stream`: one 6 x 6 array per detection."""
        return _covariances(lambda out, n: self._L.node_shell_multi_last_covariances(self._h, stream, out, n), self.max_tags)

    def rig_bundle_poses(self, max_out=8):
        """NodeOptions::rig_cameras: the rig records of the last round, one per rigid bundle."""
        out = (ShellRigBundlePose * max_out)()
        self._L.node_shell_multi_last_rig_bundle_poses.restype = C.c_int
        self._L.node_shell_multi_last_rig_bundle_poses.argtypes = [C.c_void_p, C.POINTER(ShellRigBundlePose), C.c_int]
        n = min(self._L.node_shell_multi_last_rig_bundle_poses(self._h, out, max_out), max_out)
        ints = ("status", "nobs", "nskipped", "ndropped", "ncams", "seed_stream", "seed", "chosen")
        return [dict({k: int(getattr(p, k)) for k in ints}, name=p.name.decode(), R=list(p.R), t=list(p.t), err=float(p.err),
                     sq_err_sum=float(p.sq_err_sum), R_alt=list(p.R_alt), t_alt=list(p.t_alt), err_alt=float(p.err_alt),
                     sq_err_sum_alt=float(p.sq_err_sum_alt)) for p in out[:n]]

    def rigid_bundle_covariances(self, stream, max_out=8):
        return _covariances(lambda out, n: self._L.node_shell_multi_last_rigid_covariances(self._h, stream, out, n), max_out)

    def flush(self):
        return self._L.node_shell_multi_flush(self._h)

    def publishes(self, stream):
        return self._L.node_shell_multi_publishes(self._h, stream)

    def last(self, stream):
        """(detections, header frame_id, (sec, nanosec)) of the last message published for `stream`."""
        out = (ShellDetection * self.max_tags)()
        fid = C.create_string_buffer(128)
        sec, nsec = C.c_int32(), C.c_uint32()
        n = self._L.node_shell_multi_last(self._h, stream, out, self.max_tags, fid, 128, C.byref(sec), C.byref(nsec))
        return _unpack(out, min(n, self.max_tags)), fid.value.decode(), (sec.value, nsec.value)


class AprilTagNode:
    """Parameters and defaults of the reference node (apriltag_node.cpp:564-568)."""

    def __init__(self, max_tags=64, size=0.22, tile_size=4, tag_family="tag36h11", backends="CUDA", decimate=1,
                 strict_cuapriltags_encodings=False, quad_sigma=0.0, rectify=False, resize=None, bundles=None, pose_refinement=0,
                 rigid_bundles=None, pose_covariance=0.0, raw_shift=None, tags=None, tags_listed_only=False):
        """tags, tags_listed_only (NodeOptions::tags, with pose_refinement and nothing else): [(id, size, frame)] -- every listed tag's pose
        at its own size (0: the node's) and its transform under `frame` ("": "family:id"); with tags_listed_only the other tags are
        not reported.  raw_shift (NodeOptions::raw_shift, alone among the extensions but for strict_cuapriltags_encodings): the shift of the 16-bit
        encodings' samples, 0 .. 8; the raw formats themselves ("bayer_rggb8" .. "bayer_grbg16", "mono16") are taken by every view.
        quad_sigma: AprilRobotics' blur (> 0) / sharpen (< 0) of the working image (NodeOptions::quad_sigma).  rectify
        (NodeOptions): the frames are undistorted inside the submission with the plumb_bob model of the first CameraInfo
        (on_frame: D, distortion_model, P12), and the pose is computed with Knew; "full" (NodeOptions::rectify_full): with any of the
        three distortion models and the rotation R of that CameraInfo; "corners" (NodeOptions::undistort_corners): the frames are
        detected raw and the detections' corners undistorted under that model.  resize (NodeOptions::resize_width, resize_height):
        (w, h) -- the handle has that size, frames of any size are resized to it inside the submission, behind the rectification, and
        the pose is computed with the camera scaled by w / width and h / height.  bundles (NodeOptions::bundles, alone among the
        extensions): [{"name", "members": [(id, x, y, size)], ...}] -- one "bundle:<name>" transform per solved bundle behind the tags'.
        pose_refinement (NodeOptions::pose_refinement, alone among the extensions): iterations of the orthogonal-iteration pose -- the
        detections' poses and the tags' transforms are the chosen refined pose.  rigid_bundles (NodeOptions::rigid_bundles, alone among
        the extensions): [{"name", "iterations", "members": [(id, (x, y, z), (qw, qx, qy, qz), size)], ...}] -- one "bundle:<name>"
        transform per solved rigid bundle, from the chosen pose.  pose_covariance (NodeOptions::pose_covariance_sigma_px, with
        pose_refinement and / or rigid_bundles): the corner noise in pixels -- covariances() and rigid_bundle_covariances() hand out
        what the node published."""
        rw, rh = (int(resize[0]), int(resize[1])) if resize else (0, 0)
        err = C.create_string_buffer(1024)
        self._L = lib()
        self.max_tags = max_tags
        if tags or tags_listed_only:
            if (bundles or quad_sigma or rectify or resize or rigid_bundles or pose_covariance or strict_cuapriltags_encodings
                    or raw_shift is not None):
                raise ValueError("tags is served alone by this view, or with pose_refinement")
            arr = _shell_tags(list(tags or []))
            self._h = self._L.node_shell_create_tags(max_tags, size, tile_size, tag_family.encode(), backends.encode(), decimate,
                                                     int(pose_refinement), len(tags or []), arr, 1 if tags_listed_only else 0, err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if raw_shift is not None:
            if bundles or pose_refinement or quad_sigma or rectify or resize or rigid_bundles or pose_covariance:
                raise ValueError("raw_shift is served alone by this view, or with strict_cuapriltags_encodings")
            self._h = self._L.node_shell_create_raw(max_tags, size, tile_size, tag_family.encode(), backends.encode(), decimate,
                                                    1 if strict_cuapriltags_encodings else 0, int(raw_shift), err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if pose_refinement and rectify == "corners" and not (bundles or quad_sigma or resize or rigid_bundles or strict_cuapriltags_encodings):
            # (NodeOptions::undistort_corners beside pose_refinement and, where given, pose_covariance: served together by this view)
            self._h = self._L.node_shell_create_undistort_refined(max_tags, size, tile_size, tag_family.encode(), backends.encode(), decimate,
                                                                  int(pose_refinement), float(pose_covariance), err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if pose_covariance:
            if bundles or quad_sigma or rectify or resize or strict_cuapriltags_encodings or not (pose_refinement or rigid_bundles):
                raise ValueError("pose_covariance is served with pose_refinement and / or rigid_bundles by this view, and with nothing else")
            arr = _shell_rigid_bundles(rigid_bundles or [])
            self._h = self._L.node_shell_create_covariance(max_tags, size, tile_size, tag_family.encode(), backends.encode(), decimate,
                                                           int(pose_refinement), len(arr), arr, float(pose_covariance), err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if rigid_bundles:
            if bundles or pose_refinement or quad_sigma or rectify or resize or strict_cuapriltags_encodings:
                raise ValueError("rigid_bundles is served alone by this view: not with bundles, pose_refinement, quad_sigma, rectify, resize "
                                 "or strict_cuapriltags_encodings")
            arr = _shell_rigid_bundles(rigid_bundles)
            self._h = self._L.node_shell_create_rigid_bundles(max_tags, size, tile_size, tag_family.encode(), backends.encode(), decimate,
                                                              len(arr), arr, err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if pose_refinement:
            if bundles or quad_sigma or rectify or resize or strict_cuapriltags_encodings:
                raise ValueError("pose_refinement is served alone by this view: not with bundles, quad_sigma, rectify, resize or "
                                 "strict_cuapriltags_encodings")
            self._h = self._L.node_shell_create_refined(max_tags, size, tile_size, tag_family.encode(), backends.encode(), decimate,
                                                        int(pose_refinement), err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        if bundles:
            arr = _shell_bundles(bundles)
            self._h = self._L.node_shell_create_bundles(max_tags, size, tile_size, tag_family.encode(), backends.encode(), decimate,
                                                        len(arr), arr, err, 1024)
            if not self._h:
                raise RuntimeError(err.value.decode())
            return
        self._h = self._L.node_shell_create_opts(max_tags, size, tile_size, tag_family.encode(), backends.encode(), decimate,
                                                 1 if strict_cuapriltags_encodings else 0, float(quad_sigma), _rectify_flag(rectify),
                                                 rw, rh, err, 1024)
        if not self._h:
            raise RuntimeError(err.value.decode())
        self.max_tags = max_tags

    def close(self):
        if getattr(self, "_h", None):
            self._L.node_shell_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transforms(self, max_out=128):
        """The transforms of the last published frame: the tags', then one per solved bundle."""
        out = (ShellTransform * max_out)()
        return _unpack_transforms(out, min(self._L.node_shell_last_transforms(self._h, out, max_out), max_out))

    def bundle_poses(self, max_out=8):
        out = (ShellBundlePose * max_out)()
        return _unpack_bundle_poses(out, min(self._L.node_shell_last_bundle_poses(self._h, out, max_out), max_out))

    def rigid_bundle_poses(self, max_out=8):
        out = (ShellRigidBundlePose * max_out)()
        return _unpack_rigid_bundle_poses(out, min(self._L.node_shell_last_rigid_bundle_poses(self._h, out, max_out), max_out))

    def covariances(self):
        """detection.pose.pose.covariance of the last published message: one 6 x 6 array per detection."""
        return _covariances(lambda out, n: self._L.node_shell_last_covariances(self._h, out, n), self.max_tags)

    def rigid_bundle_covariances(self, max_out=8):
        return _covariances(lambda out, n: self._L.node_shell_last_rigid_covariances(self._h, out, n), max_out)

    def on_frame(self, data_ptr, is_device, encoding, width, height, step, K9, frame_id="tf_camera", stamp=(1, 0),
                 info_stamp=None, D=None, distortion_model=None, P12=None, R=None, is_bigendian=False):
        info_stamp = stamp if info_stamp is None else info_stamp
        self._L.node_shell_set_bigendian(self._h, 1 if is_bigendian else 0)
        out = (ShellDetection * self.max_tags)()
        fid = C.create_string_buffer(128)
        err = C.create_string_buffer(1024)
        k = (C.c_double * 9)(*[float(v) for v in K9])
        d, nd, m, p = _info_extras(D, distortion_model, P12)
        n = self._L.node_shell_on_frame_full(self._h, data_ptr, 1 if is_device else 0, encoding.encode(), width, height, step, k,
                                             d, nd, m, p, _rotation(R), frame_id.encode(), stamp[0], stamp[1], info_stamp[0], info_stamp[1], out,
                                             self.max_tags, fid, 128, err, 1024)
        if n == -2:
            raise RuntimeError(err.value.decode())
        if n < 0:
            return None, None
        dets = []
        for i in range(n):
            d = out[i]
            dets.append({"id": d.id, "family": d.family.decode(), "center": list(d.center),
                         "corners": [[d.corners[c][0], d.corners[c][1]] for c in range(4)],
                         "position": list(d.position), "orientation_xyzw": list(d.orientation_xyzw),
                         "child_frame_id": d.child_frame_id.decode()})
        return dets, fid.value.decode()
