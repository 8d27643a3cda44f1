"""One handle walked through every mode of the front stage.  Rectification and resize share one pinned descriptor block, one device
block and one fill (fill_front, FrontDesc), so what can go wrong is state left over from the other mode: a stale `rectify` flag, a stale
target size, a stale camera.  Every step runs its two-frame submission twice -- captured, then replayed -- and compares the front
plane of each slot byte for byte with the CPU oracles the plane tests of tests/test_rectify_submission_gpu.py,
tests/test_resize_submission_gpu.py and tests/test_camera_models_gpu.py use.  The expected planes are tests/front_modes_cases.py's;
tests/test_front_modes_cpu.py shows without a GPU that no two steps expect the same bytes.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
import front_modes_cases as fc  # noqa: E402
import rectify_cases as rc  # noqa: E402

W, H, TARGETS = fc.W, fc.H, fc.TARGETS
INVALID_ARGUMENT = {name: code for code, name in capi.STATUS.items()}["AMDAT_INVALID_ARGUMENT"]


def _device_frame(arr, pad, offset):
    """arr in device memory with `pad` bytes (0xA5) behind every row, the first pixel `offset` bytes into the allocation."""
    h, w = arr.shape[:2]
    row = w * (arr.shape[2] if arr.ndim == 3 else 1)
    pitch = row + pad
    buf = np.full(offset + pitch * h, 0xA5, dtype=np.uint8)
    buf[offset:].reshape(h, pitch)[:, :row] = arr.reshape(h, row)
    t = torch.from_numpy(buf).cuda()
    return t, (t.data_ptr() + offset, pitch, w, h)


def _records(dets):
    return [[(d["family"], d["id"], d["hamming"], d["decision_margin"], d["p"].tobytes(), d["H"].tobytes(), d["R"].tobytes(), d["t"].tobytes())
             for d in frame] for frame in dets]


def test_one_handle_through_every_front_mode(built):
    rgb, big, planes = fc.expected()
    A, B = fc.cameras()
    keep, frames = [], {}
    for enc, srcs, pad in (("mono8", [rc.bt601(f) for f in rgb], 5), ("bgr8", [rc.encode(f, "bgr8") for f in rgb], 3),
                           ("big bgr8", [rc.encode(f, "bgr8") for f in big], 6)):
        made = [_device_frame(s, pad, 1 + i) for i, s in enumerate(srcs)]
        keep += [m[0] for m in made]
        frames[enc] = [m[1] for m in made]
    assert frames["bgr8"][0][1] == 963 and frames["big bgr8"][0][1] == 999   # (pitches that are no multiple of 4)
    k_handle, k_target = (100.0, 100.0, W / 2.0, H / 2.0), [(100.0, 100.0, t[0] / 2.0, t[1] / 2.0) for t in TARGETS]
    det = AprilTagDetector(W, H, max_batch=2, tile_size=4, decimate=1, per_frame_sizes=True)
    assert det.graph_replay()[0]

    def submit(which, intr):
        """The two-frame submission twice, captured and then replayed: ((records, threshold planes), graph nodes, per slot the debug
        planes or the codes with which they are refused), the same both times."""
        runs = []
        for _ in range(2):
            dets = det.detect_batch_ex(frames[which], max_dets=64, intrinsics=intr, encoding=which.split()[-1])
            nodes = det.last_graph_nodes()
            assert nodes > 0
            dbg = {}
            for what in (capi.DBG_RECTIFIED, capi.DBG_RESIZED):
                for slot in range(2):
                    try:
                        dbg[(what, slot)] = det.debug(slot, what).tobytes()
                    except capi.AprilTagsError as e:
                        dbg[(what, slot)] = e.code
            thresh = [det.debug(slot, capi.DBG_THRESH).tobytes() for slot in range(2)]   # (noise has no tags: the records alone say little)
            runs.append(((_records(dets), thresh), nodes, dbg))
        assert runs[0] == runs[1], "capture and replay differ (%s)" % which
        return runs[1]

    def check(step, got, formed, refused, want, shapes):
        errs = []
        for slot in range(2):
            if refused is not None and got[2][(refused, slot)] != INVALID_ARGUMENT:
                errs.append("%s: slot %d of the plane that was not formed is not refused" % (step, slot))
            if formed is None:
                continue
            plane = got[2][(formed, slot)]
            if isinstance(plane, int):
                errs.append("%s: slot %d refused with %d" % (step, slot, plane))
                continue
            dw, dh = shapes[slot]
            plane = np.frombuffer(plane, dtype=np.uint8)
            ndiff = int((plane.reshape(dh, dw) != want[slot]).sum()) if plane.size == dw * dh else -1
            print("%s slot %d: %d of %d bytes differ" % (step, slot, ndiff, dw * dh))
            if ndiff:
                errs.append("%s: slot %d, %d bytes differ" % (step, slot, ndiff))
        return errs

    same_size = ((W, H), (W, H))
    errs = []
    try:
        # 1. both modes off
        first = {enc: submit(enc, [k_handle] * 2) for enc in ("mono8", "bgr8")}
        for enc, got in first.items():
            errs += check("1 off " + enc, got, None, capi.DBG_RECTIFIED, None, None) + check("1 off " + enc, got, None, capi.DBG_RESIZED, None, None)
        nodes_off = first["mono8"][1]
        assert first["bgr8"][1] == nodes_off and first["bgr8"][0] == first["mono8"][0]   # (the fused loader: no launch more, the same gray)
        assert det.graph_replay() == (True, 2, 0)
        # 2. rectification [A, A]
        det.set_rectification([A, A])
        for enc in ("mono8", "bgr8"):
            got = submit(enc, [rc.k4(A[2])] * 2)
            assert got[1] == nodes_off + 1   # the front launch
            errs += check("2 rect AA " + enc, got, capi.DBG_RECTIFIED, capi.DBG_RESIZED, planes["rect AA"], same_size)
        assert det.graph_replay() == (True, 1, 2)   # (behind the front launch both encodings are the mono8 submission)
        # 3. resize added
        det.set_resize(list(TARGETS))
        got = submit("big bgr8", k_target)
        assert got[1] == nodes_off + 1 and det.graph_replay() == (True, 1, 3)
        errs += check("3 rect AA + resize", got, capi.DBG_RESIZED, capi.DBG_RECTIFIED, planes["rect AA + resize"], TARGETS)
        # 4. rectification off, resize still on
        det.set_rectification(None)
        got = submit("big bgr8", k_target)
        assert got[1] == nodes_off + 1 and det.graph_replay() == (True, 1, 4)
        errs += check("4 resize", got, capi.DBG_RESIZED, capi.DBG_RECTIFIED, planes["resize"], TARGETS)
        # 5. resize off, rectification [A, B]: the general kernel
        det.set_resize(None)
        det.set_rectification([A, B])
        for enc in ("mono8", "bgr8"):
            got = submit(enc, [rc.k4(A[2]), rc.k4(B[2])])
            assert got[1] == nodes_off + 1
            errs += check("5 rect AB " + enc, got, capi.DBG_RECTIFIED, capi.DBG_RESIZED, planes["rect AB"], same_size)
        assert det.graph_replay() == (True, 1, 5)   # (turning the resize off retired step 4's graph; nothing was live when the cameras came)
        # 6. both off: step 1 again
        det.set_rectification(None)
        for enc in ("mono8", "bgr8"):
            got = submit(enc, [k_handle] * 2)
            errs += check("6 off " + enc, got, None, capi.DBG_RECTIFIED, None, None) + check("6 off " + enc, got, None, capi.DBG_RESIZED, None, None)
            assert got[0] == first[enc][0] and got[1] == nodes_off, enc
        assert det.graph_replay() == (True, 2, 6)
    finally:
        det.close()
        del keep
    assert not errs, errs
