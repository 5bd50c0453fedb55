"""-m gpu: the denoiser (include/adypt_hip.h adypt_denoise ...; csrc/device/denoise.hpp, denoise.hip).  The truth is computed in this process by the numpy
restatement of the definition (tests/denoise_truth.py) from what the CPU ORACLE gives — its image, the moments of its exact per-frame samples, its
primary frames of types 0 / 4 / 5 — never from the library's read-outs; everything is compared bit for bit.  Around every call the context is what it
was, and tracing goes on to the oracle's image."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import denoise_truth as D  # noqa: E402
from tests import noise_truth as T  # noqa: E402
from tests import test_gpu_adaptive as A  # noqa: E402  (its schedule construction and its cached oracle runs)
from tests import test_gpu_noise as G  # noqa: E402     (its cases and its cached oracle runs)
from tests.helpers import bits, oracle_scene_from_instance  # noqa: E402
from tests.test_gpu_parity import make_instance  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "adypt_amd", "adypt_hip")
SEED = G.SEED
CASES = G.CASES  # tiny0 100x75 (partial blocks on two edges), tiny0 96x64 (exact blocks), sibenik 160x90 (smooth normals, many materials)
IDS = ["%s-%dx%d" % c[:3] for c in CASES]
_guides = {}


def guides_of(inst, case):
    """albedo, normal, position, hit of the oracle's primary frames (types 0, 4, 5), once per case."""
    key = case[:5]
    if key not in _guides:
        osc, P = oracle_scene_from_instance(inst), T.oracle_params(inst.m_config.c)
        frames = [O.primary_frame(osc, P, t) for t in (0, 4, 5)]
        g = dict(albedo=frames[0][0][..., :3].copy(), normal=frames[1][0][..., :3].copy(), position=frames[2][0][..., :3].copy(), hit=frames[0][1]["tri_id"] != -1)
        for v in g.values():
            v.setflags(write=False)
        _guides[key] = g
    return _guides[key]


def truth(inst, case, samples, images, n, **kw):
    """the filter on the oracle's image after n frames (n: a number, or one count per block with the image and moments per block: A.expected)"""
    g = guides_of(inst, case)
    if np.ndim(n) == 0:
        image, m2 = images[n - 1], T.moments(samples[:n])[1]
    else:
        want = A.expected(samples, images, case[1], case[2], n)
        image, m2 = want["image"], want["moments"][..., 1]
    return D.denoise(image, m2, n, g["albedo"], g["normal"], g["position"], g["hit"], **kw)


def assert_guides(got, g, tag=""):
    for k in ("albedo", "normal", "position"):
        assert np.array_equal(bits(got[k]), bits(g[k])), "%s %s" % (k, tag)
    assert np.array_equal(got["hit"], g["hit"]), "hit " + tag


def state_of(p):
    return dict(result=p.ReadResult(), moments=p.ReadNoiseMoments(), spp=p.GetSPP(), noise=p.GetNoise(), ahead=p.GetLookaheadFrames(), block_spp=p.ReadBlockSPP()[1])


def assert_same_state(a, b, tag=""):
    assert np.array_equal(bits(a["result"]), bits(b["result"])) and np.array_equal(bits(a["moments"]), bits(b["moments"])), "image / moments " + tag
    assert a["spp"] == b["spp"] and a["noise"] == b["noise"] and a["ahead"] == b["ahead"] and np.array_equal(a["block_spp"], b["block_spp"]), tag


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filter_and_guides_are_bit_exact_and_nothing_else_moves(case, scene_cache, sobol_matrices):
    name, w, h, life, sub, spp = case
    inst, _ = G._instance(scene_cache, case)
    p = inst.m_path_tracer
    samples, images = G._truth(inst, case, sobol_matrices)
    g = guides_of(inst, case)
    assert g["hit"].any() and (name != "tiny0" or not g["hit"].all())
    p.SetNoiseStats(True)
    # in the middle of a tmpLifetime group (and of the accumulation): a clobbered primary-hit cache would show in the frames that follow
    mid = life + 1 if life + 1 < spp else 5
    assert mid % life != 0 and 2 <= mid < spp
    p.Trace(True, mid)
    before, hits_before = state_of(p), p.ReadHits()
    got = p.Denoise()
    assert np.array_equal(bits(got), bits(truth(inst, case, samples, images, mid))), "Denoise() at %d spp" % mid
    assert_guides(p.ReadDenoiseGuides(), g, "at %d spp" % mid)
    assert_same_state(state_of(p), before, "around Denoise() at %d spp" % mid)
    hits_after = p.ReadHits()
    assert np.array_equal(hits_after[0], hits_before[0]) and np.array_equal(bits(hits_after[1]), bits(hits_before[1])), "the primary-hit cache moved"
    p.Trace(True, spp - mid)
    assert p.GetSPP() == spp and np.array_equal(bits(p.ReadResult()), bits(images[spp - 1])), "tracing on after Denoise() left the oracle's image"
    G._assert_moments(p, samples, spp, "after Denoise()")
    # at the case's sample count: 1, 5 and 6 levels (at 6 most taps lie outside the image), a second call, other sigmas
    before = state_of(p)
    for levels in (1, 5, 6):
        got = p.Denoise(levels=levels)
        assert np.isfinite(got).all()
        assert np.array_equal(bits(got), bits(truth(inst, case, samples, images, spp, levels=levels))), "levels %d" % levels
    again = p.Denoise(levels=6)
    assert np.array_equal(bits(again), bits(got)), "two calls in a row differ"
    got = p.Denoise(3, 1.5, 0.5)
    assert np.array_equal(bits(got), bits(truth(inst, case, samples, images, spp, levels=3, sigma_l=1.5, sigma_z=0.5)))
    assert_same_state(state_of(p), before, "around the Denoise() calls")
    ms = p.GetDenoiseTiming()
    assert len(ms["levels"]) == 3 and ms["total"] > 0.0
    p.destroy()


@pytest.mark.parametrize("variant", ["fif1", "lookahead", "launch_per_bounce"])
def test_schedules(variant, scene_cache, sobol_matrices):
    case = CASES[0]
    name, w, h, life, sub, spp = case
    inst, _ = G._instance(scene_cache, case)
    p = inst.m_path_tracer
    samples, images = G._truth(inst, case, sobol_matrices)
    p.SetNoiseStats(True)
    if variant == "lookahead":
        p.SetFramesInFlight(5)
        p.SetLookahead(True)
        for k in range(7):
            p.Trace(True, 1)
        assert p.GetLookaheadFrames() == 3  # frames 7, 8, 9 are parked: they stay parked and are handed out afterwards
    else:
        p.SetFramesInFlight(1)
        if variant == "launch_per_bounce":
            p.SetFusedBounces(False)
        p.Trace(True, 7)
    before = state_of(p)
    got = p.Denoise()
    assert np.array_equal(bits(got), bits(truth(inst, case, samples, images, 7))), variant
    assert_guides(p.ReadDenoiseGuides(), guides_of(inst, case), variant)
    assert_same_state(state_of(p), before, variant)
    for k in range(7, spp):
        p.Trace(True, 1)
    assert np.array_equal(bits(p.ReadResult()), bits(images[spp - 1])), variant
    G._assert_moments(p, samples, spp, variant)
    assert np.array_equal(bits(p.Denoise()), bits(truth(inst, case, samples, images, spp))), variant
    p.destroy()


def test_adaptive_blocks_at_their_own_sample_counts(scene_cache, sobol_matrices):
    """tiny0 100x75, target 0.1, check every 8, cap 64: blocks freeze at 8 ... 48 and one is still active (asserted by the schedule's own construction);
    the truth takes every block's image, moments and n at the block's own count."""
    case = A.TINY0
    name, w, h, life, sub, every, min_spp, cap, nominal = case
    inst, _ = A._instance(scene_cache, case)
    p = inst.m_path_tracer
    samples, images = A._truth(inst, case, sobol_matrices)
    table, target, spp_b, counter, frozen = A.plan_of(case, samples)
    spp32, counter32, frozen32 = A.schedule(table, target, every, min_spp, 32)
    assert 0 < len(frozen32) < len(spp32) and len(set(spp32.tolist())) >= 3
    p.SetNoiseStats(True)
    p.TraceAdaptive(target, min_spp, 32, every)
    before = state_of(p)
    assert np.array_equal(before["block_spp"], spp32)
    got = p.Denoise()
    assert np.array_equal(bits(got), bits(truth(inst, case, samples, images, spp32))), "Denoise() with blocks frozen"
    assert_guides(p.ReadDenoiseGuides(), guides_of(inst, case), "with blocks frozen")  # (of every owned block, not of the active ones)
    assert_same_state(state_of(p), before, "around Denoise() with blocks frozen")
    # the adaptive run goes on to where it would have gone, then plain frames of the active blocks
    r = p.TraceAdaptive(target, min_spp, cap, every)
    want = A.expected(samples, images, w, h, spp_b)
    A.assert_result(r, want, spp_b, counter, len(frozen))
    A.assert_state(p, want, spp_b, counter, w, h, "adaptive run continued after Denoise()")
    assert np.array_equal(bits(p.Denoise(levels=2)), bits(truth(inst, case, samples, images, spp_b, levels=2)))
    p.destroy()


@pytest.mark.parametrize("shape,n_dev", [((100, 75), 2), ((100, 75), 3), ((96, 64), 4), ((64, 36), 4)], ids=["100x75-2", "100x75-3", "96x64-4", "64x36-4-one-owns-nothing"])
def test_multi_device_on_one_card(shape, n_dev, scene_cache, sobol_matrices, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    w, h = shape
    case = ("tiny0", w, h, 16, 3, 9)
    inst, _ = G._instance(scene_cache, case)
    single = inst.m_path_tracer
    samples, images = G._truth(inst, case, sobol_matrices)
    c = inst.m_config
    m = api.MultiPathTracer()
    m.Initialize(c.pt_params(SEED), inst.m_hipscene, c.m_width, c.m_height, (0,) * n_dev)
    ip, iv = inst.m_camera.matrices()
    m.SetCamera(ip, iv, inst.m_camera.position)
    assert m.DeviceCount() == n_dev
    if shape == (64, 36):
        assert any(N.lib.adypt_local_pixel_count(x) == 0 for x in m._contexts())
    for t in (single, m):
        t.SetNoiseStats(True)
        t.Trace(True, 9)
    want = truth(inst, case, samples, images, 9)
    a, b = single.Denoise(), m.Denoise()
    assert np.array_equal(bits(a), bits(want)), "one context"
    assert np.array_equal(bits(b), bits(want)), "%d shards" % n_dev
    assert_guides(m.ReadDenoiseGuides(), guides_of(inst, case), "%d shards" % n_dev)
    assert np.array_equal(bits(m.Denoise(2, 2.0, 0.3)), bits(truth(inst, case, samples, images, 9, levels=2, sigma_l=2.0, sigma_z=0.3)))
    assert np.array_equal(bits(m.ReadResult()), bits(images[8])) and np.array_equal(bits(m.ReadNoiseMoments()), bits(single.ReadNoiseMoments()))
    # a shard context refuses the per-context call
    if n_dev > 1:
        with pytest.raises(N.AdyptError) as e:
            N.check(N.lib.adypt_denoise(m._contexts()[0], None), m._contexts()[0])
        assert e.value.code == N.E_STATE and "tile shard" in str(e.value)
    m.destroy()
    single.destroy()


def test_multi_device_with_blocks_frozen_at_different_counts(scene_cache, sobol_matrices, monkeypatch):
    """tiny0 100x75 on 3 shards after the adaptive run of test_adaptive_blocks_at_their_own_sample_counts (three or more freeze counts, a block still
    active): the root's images, block list and sample counts are the shards' back to back, and the filter gives the one-context result, which that test
    holds against the truth."""
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = A.TINY0
    name, w, h, life, sub, every, min_spp, cap, nominal = case
    inst, _ = A._instance(scene_cache, case)
    single = inst.m_path_tracer
    samples, images = A._truth(inst, case, sobol_matrices)
    table, target, spp_b, counter, frozen = A.plan_of(case, samples)
    spp32, counter32, frozen32 = A.schedule(table, target, every, min_spp, 32)
    assert 0 < len(frozen32) < len(spp32) and len(set(spp32.tolist())) >= 3
    c = inst.m_config
    m = api.MultiPathTracer()
    m.Initialize(c.pt_params(A.SEED), inst.m_hipscene, c.m_width, c.m_height, (0,) * 3)
    ip, iv = inst.m_camera.matrices()
    m.SetCamera(ip, iv, inst.m_camera.position)
    assert m.DeviceCount() == 3
    for t in (single, m):
        t.SetNoiseStats(True)
        t.TraceAdaptive(target, min_spp, 32, every)
    before = m.ReadBlockSPP()
    assert np.array_equal(before[1], spp32) and np.array_equal(single.ReadBlockSPP()[1], spp32)
    assert np.array_equal(bits(m.Denoise()), bits(single.Denoise())), "default parameters"
    assert np.array_equal(bits(m.Denoise(2, 2.0, 0.3)), bits(single.Denoise(2, 2.0, 0.3))), "(2, 2.0, 0.3)"
    assert_guides(m.ReadDenoiseGuides(), single.ReadDenoiseGuides(), "3 shards against one context")
    after = m.ReadBlockSPP()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]), "the sample counts moved"
    m.destroy()
    single.destroy()


def test_refusals(scene_cache):
    inst = make_instance(scene_cache, "tiny0", 96, 64)
    p = inst.m_path_tracer

    def refused(code, word, *args):
        with pytest.raises(N.AdyptError) as e:
            p.Denoise(*args)
        assert e.value.code == code and word in str(e.value), str(e.value)
    rgb = np.zeros((64, 96, 3), np.float32)
    assert N.lib.adypt_read_denoised(p._ctx, rgb.ctypes.data) == N.E_STATE and b"nothing has been denoised" in N.lib.adypt_last_error(p._ctx)
    p.Trace(True, 4)
    refused(N.E_STATE, "statistics are off")
    p.Reset()
    p.SetNoiseStats(True)
    refused(N.E_STATE, "at least 2 spp")  # 0 spp
    p.Trace(True, 1)
    refused(N.E_STATE, "at least 2 spp")  # 1 spp
    p.Trace(True, 1)
    for bad in ((0, 4.0, 0.1), (7, 4.0, 0.1), (5, 0.0, 0.1), (5, 4.0, -1.0), (5, float("nan"), 0.1)):
        refused(N.E_INVALID, "levels must be in [1, 6]", *bad)
    assert N.lib.adypt_read_denoised(p._ctx, rgb.ctypes.data) == N.E_STATE
    assert np.isfinite(p.Denoise()).all()  # 2 spp: the fewest
    assert N.lib.adypt_read_denoised(p._ctx, rgb.ctypes.data) == N.ADYPT_OK and rgb.any()
    assert N.lib.adypt_denoise(p._ctx, None) == N.ADYPT_OK  # a null pointer: the defaults
    again = np.zeros_like(rgb)
    assert N.lib.adypt_read_denoised(p._ctx, again.ctypes.data) == N.ADYPT_OK and np.array_equal(bits(again), bits(rgb))
    p.Trace(False)
    refused(N.E_STATE, "not path-traced")  # after a viewer frame
    p.destroy()
    # a context created as one of two tile shards
    part = make_instance(scene_cache, "tiny0", 100, 75, rank=1, world=2)
    q = part.m_path_tracer
    q.SetNoiseStats(True)
    q.Trace(True, 3)
    with pytest.raises(N.AdyptError) as e:
        q.Denoise()
    assert e.value.code == N.E_STATE and "tile shard" in str(e.value)
    q.destroy()


def test_cli(scene_cache, sobol_matrices, tmp_path):
    case = CASES[0]
    name, w, h, life, sub, spp = case
    inst, spec = G._instance(scene_cache, case)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    p.Trace(True, spp)
    img, den, den3, g = p.ReadResult(), p.Denoise(), p.Denoise(levels=3), p.ReadDenoiseGuides()
    p.destroy()
    out, d_exr, prefix = str(tmp_path / "o.exr"), str(tmp_path / "d.exr"), str(tmp_path / "g")

    def cli(*args):
        r = subprocess.run([CLI, spec.config_path, "--out", out, "--seed", str(SEED)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        return r.returncode, (r.stdout + r.stderr).decode()
    code, text = cli("--spp", str(spp), "--denoise", d_exr, "--guides-out", prefix)
    assert code == 0 and "Saved denoised image (5 levels)" in text, text[-2000:]
    assert np.array_equal(bits(api.load_exr(out)), bits(img)) and np.array_equal(bits(api.load_exr(d_exr)), bits(den))
    for k in ("albedo", "normal", "position"):
        assert np.array_equal(bits(api.load_exr("%s.%s.exr" % (prefix, k))), bits(g[k])), k
    code, text = cli("--spp", str(spp), "--denoise", d_exr, "--denoise-levels", "3")
    assert code == 0 and np.array_equal(bits(api.load_exr(d_exr)), bits(den3)), text[-2000:]
    # together with --noise and --adaptive: the image is the adaptive run's, the filter takes every block at its own count (finite, and not the raw image)
    code, text = cli("--spp", "32", "--noise", "0.1", "--adaptive", "--check-every", "8", "--min-spp", "8", "--denoise", d_exr)
    assert code == 0 and "[PT]ADAPTIVE" in text and "Saved denoised image" in text, text[-2000:]
    a, b = api.load_exr(out), api.load_exr(d_exr)
    assert np.isfinite(b).all() and not np.array_equal(bits(a), bits(b))
    # (what is refused before anything is loaded: tests/test_cli_options.py)
