"""Per-frame image sizes on the host (no device needed): the new entry point is exported and checks its handle, the public layouts
are what they were (the mode is a setter, not a config field), and the Python wrapper takes every frame's size from where it should."""
import ctypes as C
import os
import re

import pytest

from isaac_ros_apriltag_amd import build, capi
from isaac_ros_apriltag_amd.detector import _as_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_declared():
    L = capi.lib()
    assert "amdAprilTagsSetPerFrameSizes" in capi.EXPORTS
    assert hasattr(L, "amdAprilTagsSetPerFrameSizes")
    hdr = open(os.path.join(ROOT, "include", "apriltag_amd.h")).read()
    assert re.search(r"int amdAprilTagsSetPerFrameSizes\(amdAprilTagsHandle handle, int enable\);", hdr)


def test_null_handle_is_invalid_argument():
    L = capi.lib()
    assert L.amdAprilTagsSetPerFrameSizes(None, 1) == 1   # AMDAT_INVALID_ARGUMENT
    assert L.amdAprilTagsSetPerFrameSizes(None, 0) == 1


def test_public_layouts_are_unchanged():
    sizes = {n: C.sizeof(getattr(capi, n)) for n in ("Intrinsics", "ImageInput", "Float2", "TagID", "DetectionEx", "Config")}
    assert sizes == {"Intrinsics": 16, "ImageInput": 24, "Float2": 8, "TagID": 104, "DetectionEx": 264, "Config": 116}
    L = capi.lib()
    L.amdAprilTagsConfigLayoutVersion.restype = C.c_uint32
    assert L.amdAprilTagsConfigLayoutVersion() == 3
    cfg = capi.Config()
    L.amdAprilTagsDefaultConfig(C.byref(cfg), 640, 480)
    assert cfg.struct_size == 116


class _FakeTensor:
    """The part of a torch tensor _as_images reads."""

    def __init__(self, shape, ptr=0x1000, strides=None):
        self.shape = tuple(shape)
        if strides is None:
            strides, acc = [], 1
            for n in reversed(self.shape):
                strides.insert(0, acc)
                acc *= n
        self._strides, self._ptr = tuple(strides), ptr

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return self._strides[i]

    def data_ptr(self):
        return self._ptr

    def unsqueeze(self, d):
        assert d == 0
        return _FakeTensor((1,) + self.shape, self._ptr, (self._strides[0] * self.shape[0],) + self._strides)

    def __getitem__(self, i):
        return _FakeTensor(self.shape[1:], self._ptr + i * self._strides[0], self._strides[1:])


def _fields(arr):
    return [(int(a.width), int(a.height), int(a.dev_ptr), int(a.pitch)) for a in arr]


def test_as_images_takes_sizes_from_tensor_shapes():
    a, b = _FakeTensor((67, 1037), 0x10000), _FakeTensor((200, 300), 0x80000, (320, 1))
    arr, _ = _as_images([a, b], 1100, 200, 1, True)
    assert _fields(arr) == [(1037, 67, 0x10000, 1037), (300, 200, 0x80000, 320)]
    # the mode off: the handle's size on every frame, as before
    arr, _ = _as_images([a, b], 1100, 200)
    assert _fields(arr) == [(1100, 200, 0x10000, 1037), (1100, 200, 0x80000, 320)]
    # a stack [n, H, W], and a single [H, W]
    arr, _ = _as_images(_FakeTensor((3, 64, 96), 0x2000), 1100, 200, 1, True)
    assert _fields(arr) == [(96, 64, 0x2000 + i * 64 * 96, 96) for i in range(3)]
    arr, _ = _as_images(_FakeTensor((64, 96), 0x2000), 1100, 200, 1, True)
    assert _fields(arr) == [(96, 64, 0x2000, 96)]
    # colour: [H, W, C]
    arr, _ = _as_images([_FakeTensor((33, 40, 3), 0x3000)], 1100, 200, 3, True)
    assert _fields(arr) == [(40, 33, 0x3000, 120)]


@pytest.mark.parametrize("per_frame", (False, True))
def test_as_images_tuples(per_frame):
    """(dev_ptr, pitch, width, height) names its own size -- a window: the full image's pitch --; (dev_ptr, pitch) keeps meaning the
    handle's size."""
    arr, _ = _as_images([(0x5000 + 33 * 1100 + 517, 1100, 300, 200), (0x9000, 1152)], 1100, 200, 1, per_frame)
    assert _fields(arr) == [(300, 200, 0x5000 + 33 * 1100 + 517, 1100), (1100, 200, 0x9000, 1152)]


def test_wrong_build_is_in_the_mutant_list():
    assert 6 in build.MUTANTS and build.lib_mutant(6).endswith("libapriltag_amd_mut6.so")
    hooks = open(os.path.join(ROOT, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    assert "AMDAT_MUTATE == 6" in hooks
