"""-m gpu: what adypt_get_refit_timing, adypt_get_rebuild_timing and adypt_get_denoise_timing promise in include/adypt_hip.h, which one function
answers for all three (csrc/device/ctx_unit.hpp StageTimer::read): ADYPT_E_STATE naming the getter before there is anything to read, the number of
values and nothing written when the capacity is too small, else every value a finite time >= 0 — refit 3 stages + their total, rebuild 6 + total,
denoise 2 + levels and no total.  No durations are asserted beyond those signs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import _native as N  # noqa: E402
from tests.test_gpu_refit import case_of, pose, tracer, update  # noqa: E402

SIZE = 64
SENTINEL = -123.5


@pytest.fixture
def p(scene_cache):
    case = case_of("tiny0", scene_cache)
    t = tracer(case, case.scene, case.bvh(48), w=SIZE, h=SIZE)
    t.case = case
    yield t
    t.destroy()


def getter(name):
    return getattr(N.lib, "adypt_get_%s_timing" % name)


def nothing_yet(p, name):
    """the getter refuses with ADYPT_E_STATE, writes nothing, and the context's error names it"""
    c = p._contexts()[0]
    ms = (C.c_float * 16)(*([SENTINEL] * 16))
    r = getter(name)(c, ms, 16)
    return r == N.E_STATE and all(v == SENTINEL for v in ms) and ("adypt_get_%s_timing" % name) in (N.lib.adypt_last_error(c) or b"").decode()


def values(p, name, count, with_total):
    """the `count` values after the operation; first the call with a buffer too small for them"""
    c = p._contexts()[0]
    one = (C.c_float * 1)(SENTINEL)
    assert getter(name)(c, one, 0) == count and one[0] == SENTINEL, "%s: capacity 0 answers the count and writes nothing" % name
    ms = (C.c_float * 16)(*([SENTINEL] * 16))
    assert getter(name)(c, ms, 16) == count, name
    got = np.array(ms[:count], dtype=np.float64)
    print(name, got)
    assert all(v == SENTINEL for v in ms[count:]), "%s: nothing is written past the values" % name
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0), "%s: %s" % (name, got)
    if with_total:
        assert got[-1] > 0.0, "%s: the total" % name
    return got


def test_refit_timing(p):
    assert nothing_yet(p, "refit")
    update(p, pose(p.case.tris))
    values(p, "refit", 4, True)


def test_rebuild_timing(p):
    assert nothing_yet(p, "rebuild")
    p.RebuildBVH()
    values(p, "rebuild", 7, True)


def test_denoise_timing(p):
    p.SetNoiseStats(True)
    p.Trace(True, 2)
    assert nothing_yet(p, "denoise")
    for levels in (1, 3):
        p.Denoise(levels=levels)
        assert len(values(p, "denoise", 2 + levels, False)) == 2 + levels  # (no total entry)


def test_a_rebuild_leaves_no_refit_timing(p):
    update(p, pose(p.case.tris))
    values(p, "refit", 4, True)
    p.RebuildBVH()
    assert nothing_yet(p, "refit"), "the tree is another one: the last update's times are not to be read"
    update(p, p.case.tris)
    values(p, "refit", 4, True)
