"""The expected planes of tests/test_front_modes_gpu.py, checked without a GPU: if two steps of the walk expected the same bytes for a
slot, a step that left the previous step's plane in place would pass and the walk would prove nothing."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))

import front_modes_cases as fc  # noqa: E402


def test_no_two_steps_expect_the_same_plane(built):
    rgb, big, planes = fc.expected()   # (asserts the pairwise differences of every slot's same-shaped planes, and between the slots)
    assert [p.shape for p in planes["resize"]] == [(t[1], t[0]) for t in fc.TARGETS]
    assert [p.shape for p in planes["rect AA + resize"]] == [(t[1], t[0]) for t in fc.TARGETS]
    for name in ("rect AA", "rect AB", "rect BB"):   # every rectified plane moves most of the noise, and maps part of it outside
        for slot in range(2):
            assert planes[name][slot].shape == (fc.H, fc.W)
            assert int((planes[name][slot] != planes["source"][slot]).sum()) > fc.W * fc.H // 2
    for slot in range(2):   # the cameras differ where it matters: slot 1 of step 5 with slot 0's camera would show
        assert int((planes["rect AA"][slot] != planes["rect BB"][slot]).sum()) > fc.W * fc.H // 2
        assert not np.array_equal(planes["resize"][slot], planes["rect AA + resize"][slot])
