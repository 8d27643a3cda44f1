"""Shared helpers: run the HIP path and the CPU oracle on the same frame and compare every stage."""
import numpy as np

from isaac_ros_apriltag_amd import capi
from oracle import pyoracle as po


def oracle_params(K, decimate=1, tag_size=0.22, tile_size=4, **more):
    # the C ABI carries float intrinsics (like cuAprilTagsCameraIntrinsics_t); give the oracle the same values
    # (more: refine_edges, max_hamming, decode_sharpening, skew, quad_sigma ... -- the oracle's fields of the same names; floats as the
    # ABI's f32.  quad_sigma: the oracle filters its own working image, so `img` is the frame as submitted.)
    f32 = lambda v: float(np.float32(v))
    more = {k: (f32(v) if isinstance(v, float) else v) for k, v in more.items()}
    return po.default_params(fx=f32(K[0, 0]), fy=f32(K[1, 1]), cx=f32(K[0, 2]), cy=f32(K[1, 2]), decimate=decimate,
                             tag_size=f32(tag_size), tile_size=tile_size, **more)


def record_order(rec):
    """Indices of the records `rec` (capi.DET_DTYPE / pyoracle.RECORD_DTYPE) in the canonical preference order: family, id, lower
    hamming, higher margin, then the corner coordinates."""
    return sorted(range(len(rec)), key=lambda i: (int(rec["family"][i]), int(rec["id"][i]), int(rec["hamming"][i]),
                                                  -float(rec["decision_margin"][i])) + tuple(rec["p"][i].reshape(-1).tolist()))


def compare_records(grec, orec):
    """The decoded records BEFORE reconcile (AMDAT_DBG_DETS against the oracle's dump["dets_raw"]), both sides in the canonical order:
    counts, then every field exactly; the library's R and t are still zero there."""
    if len(grec) != len(orec):
        return ["records: gpu %d vs oracle %d" % (len(grec), len(orec))]
    g, o = grec[record_order(grec)], orec[record_order(orec)]
    for i in range(len(g)):
        for k in ("family", "id", "hamming", "decision_margin", "H", "c", "p"):
            if not np.array_equal(g[k][i], o[k][i]):
                return ["records: record %d (oracle id %d) field %s differs: %s vs %s" % (i, int(o["id"][i]), k, g[k][i].tolist(), o[k][i].tolist())]
        if g["R"][i].any() or g["t"][i].any():
            return ["records: record %d carries a pose before reconcile" % i]
    return []


def compare_stages(det, frame_idx, img, families, K, decimate=1, tag_size=0.22, verbose=False, tile_size=4, oracle=None, records=True,
                   **more):
    """Returns a list of mismatch strings (empty = bit-exact parity on every stage).  more: decode parameters the handle was created
    with beside the defaults (oracle_params).  oracle: (detections, dump) of this very frame and these parameters, where the caller
    has them already (a frame compared on both launch sets).  records=False: through the quads only -- for a stand-in frame that gives
    the oracle the library's working image but not the pixels its decode stage reads (quad_sigma at decimate > 1)."""
    errs = []
    odets, dump = oracle or po.detect(img, families=families, params=oracle_params(K, decimate, tag_size, tile_size, **more), want_dump=True)
    w, h = dump["w"], dump["h"]
    gray = det.debug(frame_idx, capi.DBG_GRAY).reshape(h, w)
    if not np.array_equal(gray, dump["gray"]):
        errs.append("gray: %d pixels differ" % int((gray != dump["gray"]).sum()))
    thr = det.debug(frame_idx, capi.DBG_THRESH).reshape(h, w)
    if not np.array_equal(thr, dump["thr"]):
        errs.append("thresh: %d pixels differ" % int((thr != dump["thr"]).sum()))
    label = det.debug(frame_idx, capi.DBG_LABEL).reshape(h, w)
    if not np.array_equal(label, dump["label"]):
        errs.append("label: %d pixels differ" % int((label != dump["label"]).sum()))
    csize = det.debug(frame_idx, capi.DBG_CSIZE).reshape(h, w)
    roots = dump["label"] == np.arange(w * h, dtype=np.uint32).reshape(h, w)
    if not np.array_equal(csize[roots], dump["csize"][roots]):
        errs.append("csize: %d roots differ" % int((csize[roots] != dump["csize"][roots]).sum()))
    counts = det.debug(frame_idx, capi.DBG_COUNTS)
    if counts[5] != 0:
        errs.append("frame flags 0x%x" % counts[5])
    cl = det.debug(frame_idx, capi.DBG_CLUSTERS)
    pts = det.debug(frame_idx, capi.DBG_POINTS)
    order = np.argsort(cl["key"], kind="stable")
    okeys = np.array([c[0] for c in dump["clusters"]], dtype=np.uint64)
    ocnt = np.array([c[2] for c in dump["clusters"]], dtype=np.uint32)
    if len(order) != len(okeys) or not np.array_equal(cl["key"][order], okeys) or not np.array_equal(cl["count"][order], ocnt):
        errs.append("clusters: gpu %d vs oracle %d (keys/counts differ)" % (len(order), len(okeys)))
    else:
        bad = 0
        for gi, (key, start, count) in zip(order, dump["clusters"]):
            g = np.sort(pts[cl["start"][gi]:cl["start"][gi] + count])
            if not np.array_equal(g, dump["points"][start:start + count]):
                bad += 1
        if bad:
            errs.append("points: %d clusters differ" % bad)
    q = det.debug(frame_idx, capi.DBG_QUADS)
    qo = np.argsort(q["key"], kind="stable")
    oq = dump["quads"]
    if len(qo) != len(oq):
        errs.append("quads: gpu %d vs oracle %d" % (len(qo), len(oq)))
    else:
        for gi, o in zip(qo, oq):
            if int(q["key"][gi]) != o["key"] or not np.array_equal(q["p"][gi], o["p"]):
                errs.append("quad key %x differs: %s vs %s" % (o["key"], q["p"][gi].tolist(), o["p"].tolist()))
                break
    if records:
        errs += compare_records(det.debug(frame_idx, capi.DBG_DETS), dump["dets_raw"])
    if verbose:
        print("   stages: clusters %d points %d quads %d dets(oracle) %d" % (len(okeys), len(dump["points"]), len(oq), len(odets)))
    return errs, odets


def compare_detections(gdets, odets, exact=True):
    errs = []
    if len(gdets) != len(odets):
        return ["detections: gpu %d vs oracle %d" % (len(gdets), len(odets))]
    for g, o in zip(gdets, odets):
        for k in ("family", "id", "hamming"):
            if g[k] != o[k]:
                errs.append("det %s: %r vs %r" % (k, g[k], o[k]))
        if np.float32(g["decision_margin"]) != np.float32(o["decision_margin"]):
            errs.append("det margin %r vs %r" % (g["decision_margin"], o["decision_margin"]))
        for k in ("H", "center", "p", "R", "t"):
            if exact:
                if not np.array_equal(g[k], o[k]):
                    errs.append("det id %d field %s differs by %.3e" % (o["id"], k, np.abs(g[k] - o[k]).max()))
            elif not np.allclose(g[k], o[k], rtol=0, atol=1e-9):
                errs.append("det id %d field %s differs by %.3e" % (o["id"], k, np.abs(g[k] - o[k]).max()))
    return errs


def _quad_crc(keys, ps, rbs):
    import zlib
    order = np.argsort(np.asarray(keys, dtype=np.uint64), kind="stable")
    crc = 0
    for i in order:
        crc = zlib.crc32(np.uint64(keys[i]).tobytes() + np.asarray(ps[i], dtype="<f4").tobytes() + np.int32(rbs[i]).tobytes(), crc)
    return crc


def stage_digest_oracle(dump):
    """Per-stage digest of an oracle dump: threshold / label CRCs, cluster and point counts, CRC of the sorted cluster list,
    number of quads and CRC of the sorted quad list (key, four float corners, border direction)."""
    import zlib
    cl = dump["clusters"]
    ck = np.array([c[0] for c in cl], dtype=np.uint64)
    cc = np.array([c[2] for c in cl], dtype=np.uint32)
    q = dump["quads"]
    return {"thr": zlib.crc32(dump["thr"].tobytes()), "label": zlib.crc32(dump["label"].tobytes()), "nclusters": len(cl),
            "npoints": int(cc.sum()), "clusters": zlib.crc32(ck.tobytes() + cc.tobytes()), "nquads": len(q),
            "quads": _quad_crc([o["key"] for o in q], [o["p"] for o in q], [o["reversed_border"] for o in q])}


def stage_digest_gpu(det, frame_idx):
    """The same digest from the library's stage buffers of frame `frame_idx` of the last submission."""
    import zlib
    cl = det.debug(frame_idx, capi.DBG_CLUSTERS)
    order = np.argsort(cl["key"], kind="stable")
    q = det.debug(frame_idx, capi.DBG_QUADS)
    return {"thr": zlib.crc32(det.debug(frame_idx, capi.DBG_THRESH).tobytes()),
            "label": zlib.crc32(det.debug(frame_idx, capi.DBG_LABEL).tobytes()), "nclusters": len(cl),
            "npoints": int(cl["count"].sum()), "clusters": zlib.crc32(cl["key"][order].tobytes() + cl["count"][order].tobytes()),
            "nquads": len(q), "quads": _quad_crc(q["key"], q["p"], q["reversed_border"])}
