"""Bayer and 16-bit frames inside the submission (k_raw_to_mono8_frames).  The definition under test: the plane a
raw frame becomes equals tests/raw_formats_ref.py byte for byte -- through the submission (AMDAT_DBG_RAW_GRAY) and through the stand-alone
call -- and every record of a raw submission is the record of the same handle given that plane as a mono8 frame, which is the CPU
oracle's record on it: on both launch sets, at every setting, with per-frame sizes, and with resize, rectification, corner undistortion
and pose refinement behind it.  The oracle-side preconditions (every detection case holds its record) are asserted in
tests/test_raw_formats_cpu.py.  Every test here fails on a library without the formats, which refuses the encodings."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
import parity_util as pu  # noqa: E402
import raw_formats_cases as cases  # noqa: E402
import raw_formats_ref as rf  # noqa: E402
import rectify_cases as rc  # noqa: E402

PATHS = ("latency", "throughput")
SETTINGS = ((1, 4, 0.0), (2, 4, 0.0), (1, 8, 0.0), (1, 4, 0.8))   # (decimate, tile_size, quad_sigma)
INVALID_ARGUMENT, UNSUPPORTED, SIZE_MISMATCH = 1, 2, 4
NSIZES = len(cases.SIZES)
WMAX, HMAX = cases.SIZES[-1][:2]
_cache = {}


def _code(fn):
    with pytest.raises(capi.AprilTagsError) as e:
        fn()
    return e.value.code


def _device_frame(arr, pad=None, offset=None):
    """arr ([H, W] uint8 or uint16) in device memory with `pad` bytes behind every row and the first sample `offset` bytes into the
    allocation -- by default an odd base address for bytes, an even one that is no multiple of 4 for 16-bit samples, and a padded
    pitch: (tensor to keep alive, (dev_ptr, pitch in bytes, width, height))."""
    two = arr.dtype.itemsize == 2
    pad = (6 if two else 5) if pad is None else pad
    offset = (2 if two else 3) if offset is None else offset
    h, w = arr.shape
    rows = np.ascontiguousarray(arr.astype("<u2") if two else arr).view(np.uint8).reshape(h, -1)
    pitch = rows.shape[1] + pad
    buf = np.full(offset + pitch * h, 0xA5, dtype=np.uint8)   # (padding that is not 0: a sample read from it would show)
    buf[offset:].reshape(h, pitch)[:, :rows.shape[1]] = rows
    t = torch.from_numpy(buf).cuda()
    return t, (t.data_ptr() + offset, pitch, w, h)


def _mono_frame(arr):
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    return t, (t.data_ptr(), arr.shape[1], arr.shape[1], arr.shape[0])


def _standalone(frame, encoding, shift, offset, pad):
    """amdAprilTagsConvertRawToMono8 into a plane `offset` bytes into its allocation with `pad` bytes behind every row: (plane, padding)."""
    ptr, pitch, w, h = frame
    dp = w + pad
    dst = torch.full((offset + dp * h,), 0x5A, dtype=torch.uint8, device="cuda")
    capi._check("amdAprilTagsConvertRawToMono8", capi.lib().amdAprilTagsConvertRawToMono8(
        ptr, pitch, capi.ENCODINGS[encoding], shift, w, h, dst.data_ptr() + offset, dp, None))
    out = dst.cpu().numpy()
    body = out[offset:].reshape(h, dp)
    return body[:, :w], np.concatenate([out[:offset], body[:, w:].reshape(-1)])


# ---- 1. the plane -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plane_handle(built):
    det = AprilTagDetector(WMAX, HMAX, max_batch=3, per_frame_sizes=True)
    yield det
    det.close()


@pytest.mark.parametrize("size", range(NSIZES), ids=["%dx%d" % s[:2] for s in cases.SIZES])
@pytest.mark.parametrize("encoding", rf.ENCODINGS)
def test_plane_bytes(plane_handle, encoding, size):
    """AMDAT_DBG_RAW_GRAY after a submission, and the stand-alone call into an aligned and into an unaligned plane, == the reference:
    noise (16-bit: over the whole range, so samples saturate at every shift below 8) and the tag frame.  The noise sits at the
    least alignment the call takes -- 8-bit sources at an odd address, 16-bit ones at an even one that is no multiple of 4 -- and
    once more, with the tag frame, at a multiple of 4 with such a pitch; every pitch is padded; 16-bit sources at shift 0, 4 and 8.
    A block is 256 x 16 pixels: 64 x 48 is three blocks of full rows, 97 x 75 and 161 x 119 have a dword tail of 1 and a last block
    of 11 and 7 rows (two blocks across: test_string_form_and_default_shift)."""
    det = plane_handle
    w, h = cases.SIZES[size][:2]
    bad = []
    for content in ("noise", "tag", "noise, aligned"):
        raw = cases.tag_frame(size, encoding) if content == "tag" else cases.noise_frame(size, encoding)
        if content == "noise":
            keep, frame = _device_frame(raw)
            assert frame[0] % (4 if rf.is16(encoding) else 2) != 0 and frame[1] > w * raw.dtype.itemsize
        else:
            keep, frame = _device_frame(raw, pad=4 + (-w * raw.dtype.itemsize) % 4, offset=0)
            assert frame[0] % 4 == 0 and frame[1] % 4 == 0 and frame[1] > w * raw.dtype.itemsize
        for shift in ((0, 4, 8) if rf.is16(encoding) else (8,)):
            want = rf.convert(raw, encoding, shift)
            if rf.is16(encoding) and content != "tag" and shift < 8:
                assert (raw >= (256 << shift)).any()   # saturating samples present
            det.set_raw_shift(shift)
            det.detect_batch_ex([frame], intrinsics=[cases.k4(w, h)], encoding=encoding)
            planes = {"submission": det.debug(0, "raw_gray").reshape(h, w)}
            planes["stand-alone, dwords"], pad_a = _standalone(frame, encoding, shift, 0, 4 - w % 4 if w % 4 else 8)
            planes["stand-alone, bytes"], pad_b = _standalone(frame, encoding, shift, 1, 5)
            assert (pad_a == 0x5A).all() and (pad_b == 0x5A).all()   # nothing written beyond a row's width
            for label, plane in planes.items():
                ndiff = int((plane != want).sum())
                print("%s %dx%d %s shift %d %s: %d of %d bytes differ" % (encoding, w, h, content, shift, label, ndiff, w * h))
                if ndiff:
                    bad.append((content, shift, label, ndiff))
        del keep
    det.set_raw_shift(8)
    assert not bad, bad


def test_string_form_and_default_shift(built):
    """amdAprilTagsConvertToMono8 takes the nine names at shift 8; a handle's default shift is 8.  517 x 35 noise: three blocks
    across, the last with a tail of 1, and three down."""
    w, h = 517, 35
    det = AprilTagDetector(w, h, max_batch=1)
    for encoding in rf.ENCODINGS:
        rng = np.random.default_rng(517)
        raw = rng.integers(0, 1 << 16, size=(h, w), dtype=np.uint16) if rf.is16(encoding) else rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        keep, (ptr, pitch, _, _) = _device_frame(raw)
        dst = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        capi._check("amdAprilTagsConvertToMono8", capi.lib().amdAprilTagsConvertToMono8(ptr, pitch, encoding.encode(), w, h, dst.data_ptr(), w, None))
        assert np.array_equal(dst.cpu().numpy(), rf.convert(raw, encoding, 8)), encoding
        det.detect_batch_ex([(ptr, pitch, w, h)], intrinsics=[cases.k4(w, h)], encoding=encoding)
        assert np.array_equal(det.debug(0, capi.DBG_RAW_GRAY).reshape(h, w), rf.convert(raw, encoding, 8)), encoding
    det.close()


# ---- 2. the records -----------------------------------------------------------------------------------------------------------------------
def _oracle(size, encoding, setting):
    key = ("o", size, encoding, setting)
    if key not in _cache:
        decimate, tile, sigma = setting
        w, h = cases.SIZES[size][:2]
        more = {"quad_sigma": sigma} if sigma else {}
        _cache[key] = po.detect(np.ascontiguousarray(cases.tag_ref(size, encoding)), families=cases.FAMILIES,
                                params=pu.oracle_params(cases.K_of(w, h), decimate, 0.22, tile, **more))[0]
    return _cache[key]


@pytest.fixture(scope="module")
def record_handles(built):
    dets = {s: AprilTagDetector(WMAX, HMAX, max_batch=3, per_frame_sizes=True, decimate=s[0], tile_size=s[1], quad_sigma=s[2], raw_shift=4)
            for s in SETTINGS}
    yield dets
    [d.close() for d in dets.values()]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("encoding", rf.ENCODINGS)
def test_records(record_handles, encoding, path):
    """A batch of three with per-frame sizes that mixes the three sizes (16-bit: 12-bit data at shift 4): detect_batch_ex(raw) == the
    same handle's records on ref(raw) as mono8 == the oracle's records on ref(raw), at decimate 1 and 2, tile 4 and 8, quad_sigma
    0.8; every list holds the record.  (The planes are test_plane_bytes' business: here the records alone decide.)"""
    order = (2, 0, 1)
    keeps, raws, monos = [], [], []
    for size in order:
        k, f = _device_frame(cases.tag_frame(size, encoding))
        k2, f2 = _mono_frame(cases.tag_ref(size, encoding))
        keeps += [k, k2]
        raws.append(f)
        monos.append(f2)
    intr = [cases.k4(*cases.SIZES[size][:2]) for size in order]
    bad = []
    for setting in SETTINGS:
        det = record_handles[setting]
        det.set_submission_path(path)
        g_raw = det.detect_batch_ex(raws, intrinsics=intr, encoding=encoding)
        g_mono = det.detect_batch_ex(monos, intrinsics=intr)
        assert det.last_submission_path() == path
        for i, size in enumerate(order):
            want = _oracle(size, encoding, setting)
            errs = pu.compare_detections(g_raw[i], g_mono[i], exact=True) + pu.compare_detections(g_raw[i], want, exact=True)
            if [(d["id"], d["hamming"]) for d in g_raw[i]] != [(cases.TAG_ID, 0)]:
                errs.append("records %s" % [(d["id"], d["hamming"]) for d in g_raw[i]])
            print("%s %s d%d-t%d-qs%g size %d: %d records, %d differ" % ((encoding, path) + setting + (size, len(g_raw[i]), len(errs))))
            if errs:
                bad.append((setting, size, errs[:3]))
    del keeps
    assert not bad, bad


# ---- 3. composition -------------------------------------------------------------------------------------------------------------------------
def _pair(encoding, size):
    """(keepalive, the raw detection case in device memory, ref(raw) as a mono8 frame in device memory)"""
    k, f = _device_frame(cases.tag_frame(size, encoding))
    k2, f2 = _mono_frame(cases.tag_ref(size, encoding))
    return (k, k2), f, f2


@pytest.mark.parametrize("encoding", rf.ENCODINGS)
def test_composition_resize_and_rectification(built, encoding):
    """Resize 161 x 119 -> 97 x 75, a mild plumb_bob rectification, and both: records and AMDAT_DBG_RESIZED / AMDAT_DBG_RECTIFIED of
    the raw run equal those of the mono8 run on ref(raw): G = convert(frame)."""
    size = 2
    w, h = cases.SIZES[size][:2]
    model = rc.model_a(w, h)
    keep, f_raw, f_mono = _pair(encoding, size)
    bad = []
    for label, kw, what, shape in (("resize", {"resize": [(97, 75)]}, capi.DBG_RESIZED, (75, 97)),
                                   ("rectify", {"rectification": [model]}, capi.DBG_RECTIFIED, (h, w)),
                                   ("rectify + resize", {"rectification": [model], "resize": [(97, 75)]}, capi.DBG_RESIZED, (75, 97))):
        det = AprilTagDetector(w, h, max_batch=1, per_frame_sizes=True, raw_shift=4, **kw)
        intr = [cases.k4(shape[1], shape[0])]
        g_raw = det.detect_batch_ex([f_raw], intrinsics=intr, encoding=encoding)[0]
        p_raw = det.debug(0, what).reshape(shape)
        G = det.debug(0, "raw_gray").reshape(h, w)
        g_mono = det.detect_batch_ex([f_mono], intrinsics=intr)[0]
        p_mono = det.debug(0, what).reshape(shape)
        assert _code(lambda: det.debug(0, "raw_gray")) == INVALID_ARGUMENT   # (the last submission was no raw one)
        det.close()
        errs = pu.compare_detections(g_raw, g_mono, exact=True)
        ndiff = int((p_raw != p_mono).sum())
        print("%s %s: %d records, %d plane bytes differ" % (encoding, label, len(g_raw), ndiff))
        if errs or ndiff or len(g_raw) != 1 or not np.array_equal(G, cases.tag_ref(size, encoding)):
            bad.append((label, len(g_raw), ndiff, errs[:3]))
    del keep
    assert not bad, bad


@pytest.mark.parametrize("encoding", rf.ENCODINGS)
def test_composition_corner_undistortion_and_refinement(built, encoding):
    """Corner undistortion with pose refinement behind a raw submission: records, undistorted twins and refined poses equal the mono8
    run's on ref(raw), field for field."""
    size = 2
    w, h = cases.SIZES[size][:2]
    K, D, Kn = rc.model_a(w, h)
    keep, f_raw, f_mono = _pair(encoding, size)
    det = AprilTagDetector(w, h, max_batch=1, raw_shift=4, corner_undistortion=[(K, D, Kn)], pose_refinement=20)
    intr = [rc.k4(Kn)]
    got = []
    for frame, enc in ((f_raw, encoding), (f_mono, "mono8")):
        g = det.detect_batch_ex([frame], intrinsics=intr, encoding=enc)[0]
        got.append((g, det.undistorted_detections(1)[0], det.refined_poses(1)[0]))
    det.close()
    del keep
    (g_raw, u_raw, r_raw), (g_mono, u_mono, r_mono) = got
    assert len(g_raw) == 1 and len(u_raw) == 1 and len(r_raw) == 1
    assert not pu.compare_detections(g_raw, g_mono, exact=True)
    for a, b in zip(u_raw + r_raw, u_mono + r_mono):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert u_raw[0]["status"] == capi.UNDISTORT_OK and r_raw[0]["status"] in (capi.POSE_REFINED, capi.POSE_REFINED_NO_ALT)


# ---- 4. graphs --------------------------------------------------------------------------------------------------------------------------------
def test_graphs_of_alternating_encodings(built):
    """One one-frame handle alternates mono8, bgr8 and bayer_grbg8 frames for three rounds: every result equals its first, the bayer
    result is the mono8 result on ref(raw) and not the result of the other mono8 frame, and the handle keeps three graphs and retires
    none (after the conversion the submission's encoding is mono8: the raw kind is part of the graph's key)."""
    size = 1
    w, h = cases.SIZES[size][:2]
    raw = cases.tag_frame(size, "bayer_grbg8")
    gray = cases.tag_gray(size)
    bgr = np.ascontiguousarray(cases.tint(gray)[..., ::-1])
    det = AprilTagDetector(w, h, max_batch=1)
    keeps = [_device_frame(raw), _mono_frame(gray), _mono_frame(cases.tag_ref(size, "bayer_grbg8"))]
    tb = torch.from_numpy(bgr).cuda()
    frames = (("mono8", [keeps[1][1]]), ("bgr8", tb), ("bayer_grbg8", [keeps[0][1]]))
    first, nodes = {}, {}
    for rnd in range(3):
        for enc, frame in frames:
            g = det.detect_batch_ex(frame, intrinsics=[cases.k4(w, h)], encoding=enc)[0]
            assert len(g) == 1 and g[0]["id"] == cases.TAG_ID
            if rnd == 0:
                first[enc], nodes[enc] = g, det.last_graph_nodes()
            else:
                assert not pu.compare_detections(g, first[enc], exact=True), (rnd, enc)
                assert det.last_graph_nodes() == nodes[enc] > 0
    on, live, retired = det.graph_replay()
    assert on and live == 3 and retired == 0
    assert nodes["bayer_grbg8"] == nodes["mono8"] + 1   # the conversion launch
    g_ref = det.detect_batch_ex([keeps[2][1]], intrinsics=[cases.k4(w, h)])[0]
    det.close()
    assert not pu.compare_detections(first["bayer_grbg8"], g_ref, exact=True)
    assert pu.compare_detections(first["bayer_grbg8"], first["mono8"], exact=True)   # (another frame: the tint shows)


def test_plane_regrows_for_a_larger_source(built):
    """With amdAprilTagsSetResize a source may exceed the handle: the plane grows before the enqueue, on a handle whose graph of the
    smaller source is live, and both sizes keep their bytes."""
    det = AprilTagDetector(97, 75, max_batch=1, resize=[(97, 75)])
    for size in (0, 2, 0, 2):
        raw = cases.noise_frame(size, "bayer_bggr8")
        h, w = raw.shape
        keep, frame = _device_frame(raw)
        det.detect_batch_ex([frame], intrinsics=[cases.k4(97, 75)], encoding="bayer_bggr8")
        assert np.array_equal(det.debug(0, "raw_gray").reshape(h, w), rf.convert(raw, "bayer_bggr8")), size
        assert np.array_equal(det.debug(0, capi.DBG_RESIZED).reshape(75, 97), po.resize_mono8(rf.convert(raw, "bayer_bggr8"), 97, 75)), size
    det.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    L = capi.lib()
    w, h = cases.SIZES[0][:2]
    det = AprilTagDetector(w, h, max_batch=1)
    intr = [cases.k4(w, h)]
    k8, f8 = _device_frame(cases.tag_frame(0, "bayer_rggb8"))
    k16, f16 = _device_frame(cases.tag_frame(0, "mono16"))
    ptr8, pitch8 = f8[:2]
    ptr16, pitch16 = f16[:2]
    sub = lambda frame, enc: det.detect_batch_ex([frame], intrinsics=intr, encoding=enc)
    det.set_raw_shift(4)
    assert len(sub(f8, "bayer_rggb8")[0]) == 1 and len(sub(f16, "mono16")[0]) == 1
    # pitch below bytes per sample x width
    assert _code(lambda: sub((ptr8, w - 1, w, h), "bayer_rggb8")) == INVALID_ARGUMENT
    assert _code(lambda: sub((ptr16, 2 * w - 2, w, h), "mono16")) == INVALID_ARGUMENT
    # an odd pointer or pitch of a 16-bit encoding
    assert _code(lambda: sub((ptr16 + 1, pitch16, w, h), "mono16")) == INVALID_ARGUMENT
    assert _code(lambda: sub((ptr16, pitch16 + 1, w, h), "bayer_bggr16")) == INVALID_ARGUMENT
    # the existing pitch limits
    assert _code(lambda: sub((ptr8, 1 << 24, w, h), "bayer_rggb8")) == INVALID_ARGUMENT
    # an encoding beyond the table
    img = (capi.ImageInput * 1)()
    img[0].width, img[0].height, img[0].dev_ptr, img[0].pitch = w, h, ptr8, pitch8
    out, cnt = (capi.DetectionEx * 8)(), (C.c_uint32 * 1)()
    assert L.amdAprilTagsDetectBatchColorEx(det._h, 1, img, 14, None, out, cnt, 8, None) == UNSUPPORTED
    # the cuAprilTagsDetect-shaped single-frame call keeps to the reference's five encodings; the batched form of one frame takes the frame
    tags, ntags = (capi.TagID * 8)(), (C.c_uint32 * 1)()
    for enc in rf.ENCODINGS:
        assert L.amdAprilTagsDetectColor(det._h, img, capi.ENCODINGS[enc], tags, ntags, 8, None) == UNSUPPORTED
    assert L.amdAprilTagsDetectBatchColor(det._h, 1, img, capi.ENCODINGS["bayer_rggb8"], None, tags, ntags, 8, None) == 0 and ntags[0] == 1
    # a Bayer source below 2 x 2 (a handle that takes such sizes through the resize); mono16 has no such limit
    dz = AprilTagDetector(w, h, max_batch=1, resize=[(w, h)])
    for ww, hh in ((1, 8), (8, 1)):
        assert _code(lambda: dz.detect_batch_ex([(ptr8, pitch8, ww, hh)], intrinsics=intr, encoding="bayer_grbg8")) == SIZE_MISMATCH
        assert _code(lambda: dz.detect_batch_ex([(ptr16, pitch16, ww, hh)], intrinsics=intr, encoding="bayer_grbg16")) == SIZE_MISMATCH
        dz.detect_batch_ex([(ptr16, pitch16, ww, hh)], intrinsics=intr, encoding="mono16")
    dz.close()
    # the roofline launch never runs a front step
    for enc in rf.ENCODINGS:
        assert _code(lambda: det.threshold_only([f16 if rf.is16(enc) else f8], encoding=enc)) == UNSUPPORTED
    # the shift: 0 .. 8, not while a submission is in flight
    assert L.amdAprilTagsSetRawShift(None, 4) == INVALID_ARGUMENT and L.amdAprilTagsSetRawShift(det._h, 9) == INVALID_ARGUMENT
    prep = det.prepare([f16], intrinsics=intr, encoding="mono16")
    det.submit_prepared(prep)
    assert L.amdAprilTagsSetRawShift(det._h, 4) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert len(det.unpack(prep)[0]) == 1   # (12-bit data at the shift the refused call did not change)
    assert L.amdAprilTagsSetRawShift(det._h, 0) == 0 and L.amdAprilTagsSetRawShift(det._h, 8) == 0
    # nothing was enqueued by a refused call: the handle still works, and the raw plane selector refuses after a mono8 submission
    assert len(sub(f8, "bayer_rggb8")[0]) == 1
    km, fm = _mono_frame(cases.tag_gray(0))
    det.detect_batch_ex([fm], intrinsics=intr)
    assert _code(lambda: det.debug(0, "raw_gray")) == INVALID_ARGUMENT
    # the stand-alone call
    dst = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    conv = lambda src, sp, enc, shift, ww, hh, dp: L.amdAprilTagsConvertRawToMono8(src, sp, enc, shift, ww, hh, dst.data_ptr(), dp, None)
    assert conv(ptr8, pitch8, capi.ENCODINGS["bayer_rggb8"], 8, w, h, w) == 0
    assert conv(ptr8, pitch8, capi.ENCODINGS["rgb8"], 8, w, h, w) == UNSUPPORTED and conv(ptr8, pitch8, 14, 8, w, h, w) == UNSUPPORTED
    assert conv(ptr16, pitch16, capi.ENCODINGS["mono16"], 9, w, h, w) == INVALID_ARGUMENT
    assert conv(ptr16 + 1, pitch16, capi.ENCODINGS["mono16"], 8, w, h, w) == INVALID_ARGUMENT
    assert conv(ptr8, w - 1, capi.ENCODINGS["bayer_rggb8"], 8, w, h, w) == INVALID_ARGUMENT
    assert conv(ptr8, pitch8, capi.ENCODINGS["bayer_rggb8"], 8, w, h, w - 1) == INVALID_ARGUMENT
    assert conv(ptr8, pitch8, capi.ENCODINGS["bayer_rggb8"], 8, 1, h, w) == SIZE_MISMATCH
    assert conv(None, pitch8, capi.ENCODINGS["bayer_rggb8"], 8, w, h, w) == INVALID_ARGUMENT
    assert L.amdAprilTagsConvertToMono8(ptr8, pitch8, b"yuv422", w, h, dst.data_ptr(), w, None) == UNSUPPORTED
    det.close()
    del k8, k16, km


# ---- 6. node shell ----------------------------------------------------------------------------------------------------------------------------
def test_node_shell_hands_raw_frames_through(built):
    """A host bayer_rggb8 frame and a host mono16 frame (12-bit data, raw_shift 4) give the detections of the mono8 frame ref(raw);
    a big-endian mono16 frame is dropped; the strict node refuses both encodings as it refuses mono8."""
    from isaac_ros_apriltag_amd import node as nd
    size = 2
    w, h = cases.SIZES[size][:2]
    K = cases.K_of(w, h)
    K9 = [K[0, 0], 0, K[0, 2], 0, K[1, 1], K[1, 2], 0, 0, 1]
    n = nd.AprilTagNode(max_tags=8, size=0.22, raw_shift=4)
    for enc in ("bayer_rggb8", "mono16"):
        raw = np.ascontiguousarray(cases.tag_frame(size, enc))
        ref = np.ascontiguousarray(cases.tag_ref(size, enc))
        d_raw, _ = n.on_frame(raw.ctypes.data, False, enc, w, h, raw.strides[0], K9)
        d_ref, _ = n.on_frame(ref.ctypes.data, False, "mono8", w, h, w, K9)
        assert [d["id"] for d in d_raw] == [cases.TAG_ID] and d_raw == d_ref, enc
    raw16 = np.ascontiguousarray(cases.tag_frame(size, "mono16"))
    assert n.on_frame(raw16.ctypes.data, False, "mono16", w, h, raw16.strides[0], K9, is_bigendian=True)[0] == []
    assert len(n.on_frame(raw16.ctypes.data, False, "mono16", w, h, raw16.strides[0], K9)[0]) == 1   # the node keeps working
    with pytest.raises(RuntimeError):
        n.on_frame(raw16.ctypes.data, False, "yuv422", w, h, 2 * w, K9)
    n.close()
    strict = nd.AprilTagNode(max_tags=8, size=0.22, strict_cuapriltags_encodings=True, raw_shift=4)
    for enc in ("bayer_rggb8", "mono16"):
        raw = np.ascontiguousarray(cases.tag_frame(size, enc))
        with pytest.raises(RuntimeError, match="only supports 'rgb8' or 'bgr8'"):
            strict.on_frame(raw.ctypes.data, False, enc, w, h, raw.strides[0], K9)
    strict.close()


# ---- 7. wrong builds ----------------------------------------------------------------------------------------------------------------------------
_SELECT = "test_plane_bytes or test_records"
_PLANE = lambda enc: ["test_plane_bytes[%s-%dx%d]" % (enc, s[0], s[1]) for s in cases.SIZES]
_WRONG_BUILDS = {
    # clamp in place of reflect at the right and bottom edge: the last column and row of every Bayer plane; mono16 has no neighbours
    49: {"must_fail": _PLANE("bayer_rggb8") + _PLANE("bayer_grbg16"), "must_pass": _PLANE("mono16")},
    # horizontal and vertical averages exchanged at the green sites of blue rows: every Bayer plane, and the records of the tinted tag
    50: {"must_fail": _PLANE("bayer_rggb8") + _PLANE("bayer_bggr16") + ["test_records[bayer_gbrg8-latency]", "test_records[bayer_grbg16-throughput]"],
         "must_pass": _PLANE("mono16") + ["test_records[mono16-latency]"]},
    # & 255 in place of the saturation: the 16-bit planes, where a sample saturates
    51: {"must_fail": _PLANE("mono16") + _PLANE("bayer_rggb16"), "must_pass": _PLANE("bayer_rggb8") + ["test_records[bayer_rggb8-latency]"]},
    # the x phase ignored in the 16-bit Bayer instance: grbg16 and bggr16 (px = 1), planes and records; the others are untouched
    52: {"must_fail": _PLANE("bayer_grbg16") + _PLANE("bayer_bggr16") + ["test_records[bayer_grbg16-latency]", "test_records[bayer_bggr16-throughput]"],
         "must_pass": _PLANE("bayer_rggb16") + _PLANE("bayer_grbg8") + ["test_records[bayer_gbrg16-latency]"]},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_raw_format_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut49.so .. _mut52.so (csrc/tools_hooks.h, AMDAT_MUTATE): the plane and record tests of this file, in a process of
    their own, must FAIL on the wrong build where its error lives, and all of them pass on the product library."""
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
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-rA", "-p", "no:cacheprovider",
                              "-k", _SELECT], capture_output=True, text=True, timeout=600, cwd=root, env=env)
        ids = lambda word: sorted(l.split("::", 1)[1].split(" ")[0] for l in out.stdout.splitlines() if l.startswith(word + " ") and "::" in l)
        return out, ids("PASSED"), ids("FAILED")
    out, passed, failed = run("mut%d" % mutant)
    assert out.returncode == 1, (out.stdout[-1500:], out.stderr[-1500:])
    for want in spec["must_fail"]:
        assert want in failed, (want, failed, passed)
    for want in spec["must_pass"]:
        assert want in passed, (want, failed, passed)
    assert "differ" in out.stdout   # what differs: bytes of the plane, records
    if "ok" not in _cache:   # (the product run is the same for every wrong build)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
