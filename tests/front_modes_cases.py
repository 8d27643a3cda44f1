"""Shared by tests/test_front_modes_cpu.py and tests/test_front_modes_gpu.py: the frames, cameras and targets of the walk through the
front stage's modes, and the CPU oracles' plane of every step and slot -- computed once per process and never changed afterwards."""
import numpy as np

from oracle import pyoracle as po
import camera_models_ref as cm
import rectify_cases as rc

W, H = 320, 48            # the handle, and the frames of the steps that do not resize
SW, SH = 331, 57          # the source frames of the resizing steps
TARGETS = ((270, 38), (320, 48))   # slot 0: no multiple of 4, not one block's extent; both cross column 256 and row 16
_cache = {}


def cameras():
    """A: plumb_bob, R = I, scaled to the handle's size as the plane tests scale it.  B: rational_polynomial behind the small rotation."""
    return rc.model_a(W, H), cm.cameras(W, H)["rational+R"]


def expected():
    """The fixed-seed noise frames and, per step and slot, the oracle's plane.  Planes of one slot that have the same shape all differ
    from one another and from the slot's source, and the slots differ: a step that left the previous step's plane, or another
    slot's, cannot pass."""
    if "exp" not in _cache:
        rng = np.random.default_rng(32048)
        rgb = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(2)]
        big = [rng.integers(0, 256, size=(SH, SW, 3), dtype=np.uint8) for _ in range(2)]
        gray, gbig = [rc.bt601(f) for f in rgb], [rc.bt601(f) for f in big]
        A, B = cameras()
        planes = {
            "source": gray,
            "rect AA": [po.rectify_mono8(g, *A) for g in gray],
            "rect AA + resize": [po.resize_mono8(po.rectify_mono8(g, *A), *t) for g, t in zip(gbig, TARGETS)],
            "resize": [po.resize_mono8(g, *t) for g, t in zip(gbig, TARGETS)],
            "rect AB": [po.rectify_mono8(gray[0], *A), cm.rectify(gray[1], *B)],
            "rect BB": [cm.rectify(g, *B) for g in gray],   # (not a step: what slot 0 would be with slot 1's camera)
        }
        names = sorted(planes)
        for slot in range(2):
            for i, a in enumerate(names):
                for b in names[i + 1:]:
                    pa, pb = planes[a][slot], planes[b][slot]
                    same_on_purpose = {a, b} == ({"rect AA", "rect AB"} if slot == 0 else {"rect AB", "rect BB"})
                    if pa.shape == pb.shape and not same_on_purpose:
                        assert not np.array_equal(pa, pb), (slot, a, b)
        for a in names:
            if planes[a][0].shape == planes[a][1].shape:
                assert not np.array_equal(planes[a][0], planes[a][1]), a
        assert np.array_equal(planes["rect AA"][0], planes["rect AB"][0])
        _cache["exp"] = (rgb, big, planes)
    return _cache["exp"]
