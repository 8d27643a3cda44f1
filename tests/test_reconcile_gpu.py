"""k_reconcile on records the test chooses (amdAprilTagsDebugReconcile): every case of tests/reconcile_cases.py equals the plain Python
statement (tests/reconcile_ref.py) and the oracle's ato_reconcile exactly -- kept set, order, every field, R and t included.  The
handle holds 256 records: the random cases of 65, 130 and 256 records take the rank sort's second to fourth trip.  Afterwards the same
handle detects a frame as the oracle does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
import parity_util as pu  # noqa: E402
import reconcile_cases as rcs  # noqa: E402

expected_records, params, same_records = rcs.expected_records, rcs.params, rcs.same_records


@pytest.fixture(scope="module")
def handle(built):
    det = AprilTagDetector(640, 480, families=("tag36h11", "tag25h9"), decimate=2, intrinsics=rcs.INTRINSICS, tag_size=rcs.TAG_SIZE,
                           max_batch=1, max_detections=rcs.MAX_DETECTIONS)
    yield det
    det.close()


def _check(det, records):
    got = det.debug_reconcile(records)
    want_ref, want_oracle = expected_records(records), po.reconcile(records, params())
    assert same_records(want_ref, want_oracle)
    assert len(got) == len(want_ref), (len(got), len(want_ref), got[["id", "hamming", "decision_margin"]], want_ref[["id", "hamming", "decision_margin"]])
    for f in got.dtype.names:
        assert np.array_equal(got[f], want_ref[f]), (f, got[f][:4], want_ref[f][:4])
    assert same_records(got, want_ref)


@pytest.mark.parametrize("name", sorted(rcs.CRAFTED))
def test_crafted_case(handle, name):
    _check(handle, rcs.crafted(name)[0])


@pytest.mark.parametrize("n", rcs.RANDOM_COUNTS)
def test_random_case(handle, n):
    _check(handle, rcs.random_case(n))


def test_more_records_than_the_handle_holds_are_refused_and_the_handle_still_detects(handle):
    too_many = np.concatenate([rcs.random_case(rcs.MAX_DETECTIONS), rcs.random_case(1)])
    with pytest.raises(capi.AprilTagsError) as e:
        handle.debug_reconcile(too_many)
    assert capi.STATUS[e.value.code] == "AMDAT_INVALID_ARGUMENT"
    _check(handle, rcs.random_case(130))
    with pytest.raises(capi.AprilTagsError):   # nothing of a submission to inspect behind a reconcile of its own
        handle.debug(0, capi.DBG_COUNTS)
    # the handle afterwards: a frame detected as the oracle detects it, every stage and the records
    img, _, _ = synth.scene_c1()
    fx, fy, cx, cy = rcs.INTRINSICS
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    fams = ("tag36h11", "tag25h9")
    frame = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    for _ in range(2):   # captured, then replayed
        g = handle.detect_batch_ex(frame)[0]
        errs, odets = pu.compare_stages(handle, 0, img, fams, K, decimate=2, tag_size=rcs.TAG_SIZE)
        errs += pu.compare_detections(g, odets)
        assert not errs and len(g) == 1, errs
        _check(handle, rcs.crafted("chain_c_survives")[0])
