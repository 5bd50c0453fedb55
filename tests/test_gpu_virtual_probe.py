"""-m gpu: k_temporal_merge_virtual (csrc/device/denoise_kernels.hpp) alone, on the hand-made edge images of tests/virtual_edge_inputs.py at 33 x 9 — one
column and one row more than its 32 x 8 workgroup — through adypt_amd/libadypt_probe.so, which launches it with the launch shape the product uses.
Compared with probe.same (equal bits, or NaN on both sides) against tests/virtual_truth.py; every output is filled with a sentinel word before the
launch, and every pixel must have lost it; every case reaches what it is named after by the truth's account."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import probe as P  # noqa: E402
from tests import virtual_edge_inputs as E  # noqa: E402

F = np.float32
CASES = E.cases((33, 9))


def merge_virtual(case):
    """k_temporal_merge_virtual: (merged (h, w, 4), X2 as the kernel leaves it, length (h, w), (followed, with history))"""
    h, w = case["h"], case["w"]
    imgs = [P._img(case[k], h, w) for k in ("x0", "x1", "x2", "xa", "xv", "h0", "h1", "h2", "ha")]
    o, ip, iv = (P._f(v) for v in case["cam"])
    merged, x2, length, counts = np.empty((h, w, 4), F), np.empty((h, w, 4), F), np.empty((h, w), F), np.zeros(2, np.uint64)
    P._call("temporal_merge_virtual", *imgs, C.c_int(case["have"]), o, ip, iv, C.c_float(case["cap"]), C.c_int(w), C.c_int(h), merged, x2, length, counts)
    return merged, x2, length, (int(counts[0]), int(counts[1]))


@pytest.mark.parametrize("name", list(CASES))
def test_merge_by_the_virtual_point(name):
    case = CASES[name]
    Dm, Vm, no, followed, with_history = E.truth(case)
    assert case["reach"](no), "the case does not reach what it is named after"
    merged, x2, length, counts = merge_virtual(case)
    for what, got, want in (("merged D", merged[..., :3], Dm), ("merged V", merged[..., 3], Vm), ("length", length, no), ("X2.w", x2[..., 3], no), ("X2.xyz", x2[..., :3], case["x2"][..., :3])):
        got = np.ascontiguousarray(got, dtype=F)
        assert not P.unwritten(got).any(), "%s: %s has words no thread wrote" % (name, what)
        ok = P.same(got, want)
        assert ok.all(), "%s: %d words of %s differ, the first at %s" % (name, int((~ok).sum()), what, np.argwhere(~ok)[0].tolist())
    assert counts == (followed, with_history), "%s: counted %s, the truth %s" % (name, counts, (followed, with_history))
