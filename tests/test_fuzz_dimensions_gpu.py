"""The fuzzer's dimensions beyond the plain one (tools/fuzz_gpu.py: run_cases), each alone and all of them together: colour
submissions, tile 8, random decode parameters, a base address and a pitch of its own per frame, a random quad_sigma -- and their
interactions (a colour frame at an odd address under tile 8 with random decode parameters and a filter; three frames of mixed
alignment in one launch), where a per-frame `aligned` flag or a descriptor pointer goes wrong.  Even cases run the latency launch set,
odd cases the throughput set.  Every stage and every record of every frame bit-identical to the oracle."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ALL = dict(colour=True, params=True, layout=True, quad_sigma=True)

# name -> (cases, seed, maxdim, run_cases arguments).  The seeds of the tile-8 calls were checked with a dry run of the generator:
# the cases they leave out (a working image below 8 pixels a side, which the library refuses by design) stay below the cap.
CALLS = {
    "colour": (100, 20261001, 300, dict(colour=True)),
    "tile8": (100, 20261002, 300, dict(tile=8)),
    "params": (100, 20261003, 300, dict(params=True)),
    "layout": (100, 20261004, 300, dict(layout=True)),
    "quad_sigma": (100, 20261005, 300, dict(quad_sigma=True)),
    "all_tile4": (100, 20261006, 280, dict(ALL, tile=4)),
    "all_tile8": (100, 20261007, 280, dict(ALL, tile=8)),
    "all_batch3": (40, 20261008, 260, dict(ALL, tile=4, batch=3)),
}


def _fuzzer():
    spec = importlib.util.spec_from_file_location("fuzz_gpu", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_gpu.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    return fz


@pytest.mark.parametrize("name", list(CALLS))
def test_fuzz_dimension(built, name):
    cases, seed, maxdim, kw = CALLS[name]
    stats = {}
    done, fails = _fuzzer().run_cases(cases, seed=seed, maxdim=maxdim, out=lambda m: None, path="alternate", stats=stats, **kw)
    assert not fails, fails[:3]
    left_out = stats["left_out"]
    if kw.get("tile", 4) == 8:
        # the size generator alone leaves out 12-13 % on average at these maxdim; a quarter is more than three standard deviations
        # away at 100 cases
        assert done + left_out == cases and 4 * left_out <= cases, (done, left_out)
    else:
        assert done == cases and left_out == 0, (done, left_out)
