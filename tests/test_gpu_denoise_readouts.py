"""-m gpu: how long the denoiser's read-outs live (include/adypt_hip.h adypt_read_denoise_..., adypt_get_denoise_...).  The rule, stated here and not
taken from the library: a read-out answers from the first call of its kind that ran to its end and keeps answering whatever calls follow; the info
structs say what the last call OF THAT KIND was given, not the last call; the merge time answers only while the last call had history.  The seven
kinds of call are made on one context in an order that interleaves them, and after each every read-out is asked."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import _native as N  # noqa: E402
from tests.test_gpu_parity import make_instance  # noqa: E402

W, H = 72, 40  # no multiple of the 32 x 32 block in either direction

# (the kind, Denoise's arguments), in the order they are made: a plain call between two temporal ones, a moments call between two rectified ones
CALLS = [("plain", dict()),
         ("temporal", dict(temporal=True)),
         ("plain", dict(levels=2)),
         ("temporal", dict(temporal=True, commit=False)),
         ("rectified", dict(temporal=True, rectify=True, rectify_radius=2, rectify_gamma=0.5)),
         ("moments", dict(temporal=True, moments=True)),
         ("rectified", dict(temporal=True, rectify=True, rectify_radius=1, rectify_gamma=2.0)),
         ("specular", dict(specular_bounces=2)),
         ("motion", dict(temporal=True, follow_motion=True)),
         ("temporal-specular", dict(temporal=True, follow_specular=3)),
         ("specular", dict(specular_bounces=5)),
         ("plain", dict()),
         ("rectified", dict(temporal=True, rectify=True)),
         ("temporal-specular", dict(temporal=True, follow_specular=1, commit=False)),
         ("moments", dict(temporal=True, moments=True, follow_motion=True)),
         ("temporal", dict(temporal=True))]
WITH_HISTORY = ("temporal", "motion", "rectified", "moments", "temporal-specular")

# what each read-out says while no call of its kind has run, behind "<entry>: "
NONE_YET = {"history": ("adypt_read_denoise_history", "no temporal call has run yet (adypt_denoise_temporal)"),
            "motion": ("adypt_read_denoise_motion", "no motion call has run yet (adypt_denoise_temporal_motion)"),
            "rectify": ("adypt_read_denoise_rectify", "no rectified call has run yet (adypt_denoise_temporal_rectified)"),
            "variance": ("adypt_read_denoise_variance", "no moments call has run yet (adypt_denoise_temporal_moments)"),
            "virtual": ("adypt_read_denoise_virtual", "no call by the virtual point has run yet (adypt_denoise_temporal_specular)"),
            "merge_ms": ("adypt_get_denoise_merge_ms", "the last filter was not a temporal call (adypt_denoise_temporal)")}


def expected_after(calls):
    """The rule above, applied to the calls made so far: which read-outs answer, and what the info structs hold."""
    want = dict(history=False, motion=False, rectify=None, variance=False, virtual=None, chain=None, merge_ms=False, snapshot=False)
    for kind, kw in calls:
        want["merge_ms"] = kind in WITH_HISTORY
        if kind in WITH_HISTORY:
            want["history"] = True
            if kw.get("commit", True):  # the snapshot belongs to the history: a committing call leaves one exactly when it follows motion
                want["snapshot"] = bool(kw.get("follow_motion"))
        if kw.get("follow_motion"):
            want["motion"] = True
        if kind == "rectified":
            want["rectify"] = (kw.get("rectify_radius", 3), kw.get("rectify_gamma", 1.0))
        if kind == "moments":
            want["variance"] = True
        if kind == "temporal-specular":
            want["virtual"] = want["chain"] = kw["follow_specular"]
        if kind == "specular":
            want["chain"] = kw["specular_bounces"]
    return want


def answers(p, name, read, expect):
    """read() answers, or raises ADYPT_E_STATE with exactly the read-out's text"""
    if expect:
        return read()
    with pytest.raises(N.AdyptError) as e:
        read()
    assert e.value.code == N.E_STATE and str(e.value) == "ADYPT_E_STATE (%d): %s: %s" % ((N.E_STATE,) + NONE_YET[name]), (name, str(e.value))
    return None


def check_readouts(p, want, tag):
    n = answers(p, "history", p.ReadDenoiseHistory, want["history"])
    assert n is None or (n.shape == (H, W) and (n >= 1.0).all()), tag
    m = answers(p, "motion", p.ReadDenoiseMotion, want["motion"])
    assert m is None or (m["previous_position"].shape == (H, W, 3) and m["moved"].shape == (H, W)), tag
    k = answers(p, "rectify", p.ReadDenoiseRectify, want["rectify"] is not None)
    assert k is None or k.shape == (H, W), tag
    v = answers(p, "variance", p.ReadDenoiseVariance, want["variance"])
    assert v is None or v.shape == (H, W), tag
    x = answers(p, "virtual", p.ReadDenoiseVirtual, want["virtual"] is not None)
    assert x is None or (x["virtual_position"].shape == (H, W, 3) and (x["distance"] >= 0.0).all()), tag
    ms = answers(p, "merge_ms", p.GetDenoiseMergeMs, want["merge_ms"])
    assert ms is None or ms > 0.0, tag
    # the info calls always answer; `have` and the parameters are those of the last call of the kind
    info = p.GetDenoiseMotion()
    assert info["have_snapshot"] == (1 if want["snapshot"] else 0) and (info["n_tris"] > 0) == want["snapshot"], (tag, info)
    assert (info["device_bytes"] > 0) == want["motion"], (tag, info)
    info = p.GetDenoiseRectify()
    if want["rectify"] is None:
        assert (info["have"], info["radius"], info["gamma"], info["device_bytes"]) == (0, 0, 0.0, 0), (tag, info)
    else:
        assert (info["have"], info["radius"], info["gamma"]) == (1,) + want["rectify"] and info["device_bytes"] >= 36 * W * H and info["window_ms"] > 0.0, (tag, info)
    info = p.GetDenoiseMoments()
    assert info["have"] == (1 if want["variance"] else 0) and (info["device_bytes"] > 0) == want["variance"], (tag, info)
    assert not want["variance"] or (info["variance_ms"] > 0.0 and 0 <= info["pixels_spatial"] <= W * H), (tag, info)
    info = p.GetDenoiseVirtual()
    assert (info["have"], info["bounces"]) == ((1, want["virtual"]) if want["virtual"] else (0, 0)) and (info["device_bytes"] > 0) == bool(want["virtual"]), (tag, info)
    assert info["pixels_with_history"] <= info["pixels_followed"] <= W * H, (tag, info)
    info = p.GetDenoiseSpecular()
    assert (info["have"], info["bounces"]) == ((1, want["chain"]) if want["chain"] else (0, 0)) and (info["device_bytes"] > 0) == bool(want["chain"]), (tag, info)
    assert not want["chain"] or info["chain_ms"] > 0.0, (tag, info)


def test_every_readout_after_every_kind_of_call(scene_cache):
    assert {k for k, _ in CALLS} == {"plain", "temporal", "motion", "rectified", "moments", "specular", "temporal-specular"}
    inst = make_instance(scene_cache, "tiny0", W, H)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    p.Trace(True, 2)
    check_readouts(p, expected_after([]), "before the first call")
    for k, (kind, kw) in enumerate(CALLS):
        rgb = p.Denoise(**kw)
        assert rgb.shape == (H, W, 3) and np.isfinite(rgb).all(), (k, kind)
        check_readouts(p, expected_after(CALLS[:k + 1]), "after call %d (%s)" % (k, kind))
    p.destroy()
