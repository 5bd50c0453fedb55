"""-m gpu: the kernels of a moments call and the three later prepare instances (csrc/device/denoise_kernels.hpp) ONE BY ONE on the hand-made edge images
of tests/moments_edge_inputs.py, through adypt_amd/libadypt_probe.so (tests/probe.py), which launches each kernel once with the launch shape the product
uses: k_denoise_prepare_class / _moments / _virtual, k_temporal_merge_moments<false | true> and k_moments_variance.  The conventions are
tests/test_gpu_denoise_probes.py's: probe.same against the numpy truths with no tolerance, every output pre-filled with a sentinel word that every
pixel must have lost, every case proven to reach its branch from its inputs or from the truth's side (tests/test_moments_definition.py holds the same
cases against the headers on the CPU)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import denoise_edge_inputs as E  # noqa: E402
from tests import moments_edge_inputs as M  # noqa: E402
from tests import probe as P  # noqa: E402
from tests.test_gpu_denoise_probes import check  # noqa: E402

F = np.float32
PREPARE, MERGE, VARIANCE = M.prepare_cases(), M.merge_cases(), M.variance_cases()


# ---- k_denoise_prepare_class, k_denoise_prepare_moments, k_denoise_prepare_virtual ----
def _prepare_params():
    out = []
    for name, case in PREPARE.items():
        seen = []
        for order_name, order in E.block_orders(case["w"], case["h"]).items():
            if tuple(order) not in seen:
                seen.append(tuple(order))
                out += [pytest.param(name, order_name, instance, id="%s-%s-%s" % (instance, name, order_name)) for instance in P.PREPARE_INSTANCES]
    return out


@pytest.mark.parametrize("name, order_name, instance", _prepare_params())
def test_prepare_instances(name, order_name, instance):
    case = PREPARE[name]
    assert M.prepare_reach(case, instance), "the case does not reach what it is named after"
    w, h = case["w"], case["h"]
    order = E.block_orders(w, h)[order_name]
    if order_name != "ascending":
        assert not np.array_equal(order, np.sort(order)), "the block list is the ascending one"
    inp = M.prepare_inputs(case, order)
    assert inp["pad"].sum() == len(order) * 1024 - w * h and (len(set(inp["block_spp"].tolist())) > 1 or len(order) == 1), "pixels outside the picture; a count per block"
    got = P.denoise_prepare_instance(instance, inp["accum"], inp["moments"], inp["albedo"], inp["normal"], inp["position"], inp["hits"], inp["blocks"], inp["block_spp"], w, h,
                                     virtual=inp["virtual"] if instance == "virtual" else None)
    want = M.prepare_truth(case, instance)
    assert len(got) == len(want)
    for k, (g, t) in enumerate(zip(got, want)):
        check(g, t, "%s, %s, blocks %s: %s" % (instance, name, order_name, ("X0", "X1", "X2", "XA", "XV")[k]))
        assert not (g == M.POISON).any(), "a word of a local pixel outside the picture"


# ---- k_temporal_merge_moments<false>, <true> ----
@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
@pytest.mark.parametrize("key", list(MERGE))
def test_merge_moments(key, motion):
    case = MERGE[key]
    assert case["reach"](M.merge_truth(case)), "the case does not reach what it is named after"
    im = E.images(case["call"])
    h, w = im["hit"].shape
    hist, cap = case["hist"], case["kw"].get("cap", 64.0)
    _, XP, XN, _ = M.merge_through(case)
    # (the plain instance of a motion case merges through the pixel's own N and P: MT.merge without `through`)
    t = M.merge_truth(dict((k, v) for k, v in case.items() if motion or k != "tri"), motion=motion)
    # (a call without a history is given what lies in the history's memory all the same — "stale", as after a reset — and told that there is none)
    H, raw = E.h_images(hist if hist is not None else case.get("stale"), h, w)
    merged, x2, length = P.temporal_merge_moments(E.x_images(im), H, hist is not None, raw, cap, motion=(XP, XN) if motion else None)
    what = "%s, motion %s: " % (key, motion)
    check(merged, E.rgba(t["D"], t["V"]), what + "the merged image")
    check(x2, E.rgba(im["P"], t["n_out"]), what + "X2 with n_out")
    check(length, t["n_out"], what + "the history length")


# ---- k_moments_variance ----
@pytest.mark.parametrize("name", list(VARIANCE))
def test_variance(name):
    case = VARIANCE[name]
    t = M.variance_truth(case)
    assert case["reach"](t), "the case does not reach what it is named after"
    out, variance, count = P.moments_variance(*M.variance_images(case), case["origin"])
    check(out, E.rgba(case["D"], t["V"]), name + ": (D, V)")
    check(variance, t["V"], name + ": the variance read-out")
    assert count == int(t["spatial"].sum()), "%s: counted %d pixels that took the window estimate, the truth %d" % (name, count, int(t["spatial"].sum()))
