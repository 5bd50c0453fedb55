"""-m gpu: the noise statistics (include/adypt_hip.h adypt_set_noise_stats ... adypt_trace_until; csrc/device/noise.hpp).  The truth is computed
in this process from the CPU oracle's exact per-frame samples and the numpy restatement of the definition (tests/noise_truth.py), never taken
from the library: moments and per-pixel noise bit for bit, block sums and image numbers within 2^-40 relative (1023 additions of non-negative
binary64 values in any order differ by less than 1023 x 2^-53 < 2^-43; three bits of margin).  In every run the image stays the oracle's."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import noise_truth as T  # noqa: E402
from tests.helpers import bits, oracle_scene_from_instance  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "adypt_amd", "adypt_hip")
REL = 2.0 ** -40
SEED = 31

#        scene      w    h   life sub spp
CASES = [("tiny0", 100, 75, 16, 3, 16),     # partial blocks at the right and bottom edge; all frames inside the first tmpLifetime group
         ("tiny0", 96, 64, 4, 1, 37),       # no sub-pixel jitter: every frame's CPU sample is exact
         ("sibenik", 160, 90, 3, 1, 20)]
UNTIL = ("tiny0", 96, 64, 4, 1, 64)
_truth_cache = {}


def _instance(cache, case):
    name, w, h, life, sub, _ = case
    spec = scenes.make_scene(name, cache, width=w, height=h, pt={"tmpLifetime": life, "maxBounce": 6, "subpixel": sub})
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=SEED), api.InstanceConfig.last_error()
    return inst, spec


def _truth(inst, case, sobol_matrices, sun=False, n=None):
    """(samples of every frame, the oracle's image after every frame) of a case, computed once per session."""
    n = case[5] if n is None else n
    key = case[:5] + (n, sun)
    if key not in _truth_cache:
        c = inst.m_config.c
        osc, P, shift = oracle_scene_from_instance(inst), T.oracle_params(c, sun), O.shift_bytes(SEED, c.width, c.height)
        samples = T.frame_samples(osc, P, shift, sobol_matrices, n)
        state, images = O.PathTracerState(c.width, c.height), []
        for _ in range(n):
            O.pt_frames(osc, P, shift, sobol_matrices, state, 1)
            images.append(state.accum[..., :3].copy())
        _truth_cache[key] = (samples, images)
    return _truth_cache[key]


def _assert_moments(p, samples, n, tag=""):
    mean, m2 = T.moments(samples[:n])
    got = p.ReadNoiseMoments()
    assert np.array_equal(bits(got[..., 0]), bits(mean)), "mean after %d frames %s" % (n, tag)
    assert np.array_equal(bits(got[..., 1]), bits(m2)), "m2 after %d frames %s" % (n, tag)


def _close(a, b):
    return abs(a - b) <= REL * abs(b)


def _assert_readouts(p, samples, n, w, h):
    t = T.truth(samples, n)
    print("truth after %d frames: mean_noise %.6f worst_block %.6f worst_index %d gap %.3g" % (n, t["mean_noise"], t["worst_block"], t["worst_index"], t["gap"]))
    assert np.array_equal(bits(p.ReadNoise()), bits(t["e"]))
    idx, s, cnt = p.ReadBlockNoise()
    assert np.array_equal(idx, t["idx"]) and np.array_equal(cnt, t["count"]) and int(cnt.sum()) == w * h
    rel = np.abs(s - t["sum"]) / np.maximum(t["sum"], np.finfo(np.float64).tiny)
    print("largest relative error of a block sum: %.3g (bound %.3g)" % (rel.max(), REL))
    assert (rel <= REL).all()
    g = p.GetNoise()
    assert g["spp"] == n and g["pixels"] == w * h
    assert _close(g["mean_noise"], t["mean_noise"]) and _close(g["worst_block"], t["worst_block"])
    assert t["gap"] > 2 * REL * t["worst_block"], "the case does not separate its two noisiest blocks"
    assert g["worst_index"] == t["worst_index"]
    # two queries in a row: identical bits
    g2 = p.GetNoise()
    idx2, s2, cnt2 = p.ReadBlockNoise()
    assert g2 == g and np.array_equal(s2.view(np.uint64), s.view(np.uint64)) and np.array_equal(cnt2, cnt)
    return g


@pytest.mark.parametrize("variant", ["fif1", "fif5", "fif32", "lookahead", "launch_per_bounce", "sun_visibility"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-life%d-sub%d-%dspp" % c)
def test_moments_are_bit_exact_and_the_image_is_untouched(case, variant, scene_cache, sobol_matrices):
    name, w, h, life, sub, spp = case
    inst, _ = _instance(scene_cache, case)
    p = inst.m_path_tracer
    sun = variant == "sun_visibility"
    samples, images = _truth(inst, case, sobol_matrices, sun)
    p.SetNoiseStats(True)
    assert p.GetNoiseStats()
    if variant == "lookahead":
        p.SetFramesInFlight(5)
        p.SetLookahead(True)
        for k in range(spp):  # one frame per call, checked after EVERY call: the moments follow the frames handed out, not the frames traced ahead
            p.Trace(True, 1)
            assert p.GetSPP() == k + 1 and p.GetLookaheadFrames() == (5 - 1 - k % 5)
            _assert_moments(p, samples, k + 1, "(look-ahead)")
            assert np.array_equal(bits(p.ReadResult()), bits(images[k])), "image after call %d" % k
    else:
        if variant.startswith("fif"):
            p.SetFramesInFlight(int(variant[3:]))
        if variant == "launch_per_bounce":
            p.SetFramesInFlight(1)
            p.SetFusedBounces(False)  # the lone launch-per-bounce frame: with the statistics on its sample is parked and resolved
        if sun:
            p.SetSunVisibility(True)
        p.Trace(True, spp - 3)
        _assert_moments(p, samples, spp - 3, variant)
        p.Trace(True, 3)  # the accumulation continues across calls
        assert p.GetSPP() == spp
        if variant == "launch_per_bounce":
            assert not p.GetFusedBounces()
        _assert_moments(p, samples, spp, variant)
        assert np.array_equal(bits(p.ReadResult()), bits(images[spp - 1])), "the statistics changed the picture (%s)" % variant
    p.destroy()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-life%d-sub%d-%dspp" % c)
def test_noise_readouts(case, scene_cache, sobol_matrices):
    name, w, h, life, sub, spp = case
    inst, _ = _instance(scene_cache, case)
    p = inst.m_path_tracer
    samples, images = _truth(inst, case, sobol_matrices)
    p.SetNoiseStats(True)
    p.Trace(True, 2)
    _assert_readouts(p, samples, 2, w, h)  # the fewest frames the estimate is defined for
    p.Trace(True, spp - 2)
    _assert_readouts(p, samples, spp, w, h)
    assert np.array_equal(bits(p.ReadResult()), bits(images[spp - 1]))
    p.destroy()


def test_sub_pixel_jitter_beyond_the_first_group(scene_cache, sobol_matrices):
    """tmpLifetime 2, subpixel 3, 20 spp: from frame 2 on there are no exact CPU samples, so the schedules are held against each other; the first
    2 spp against the numpy truth."""
    case = ("tiny0", 72, 40, 2, 3, 20)
    ref = None
    for fif in (1, 8, 32):
        for lookahead in (False, True):
            inst, _ = _instance(scene_cache, case)
            p = inst.m_path_tracer
            p.SetFramesInFlight(fif)
            p.SetLookahead(lookahead)
            p.SetNoiseStats(True)
            p.Trace(True, 2)
            samples, images = _truth(inst, case, sobol_matrices, n=2)
            _assert_moments(p, samples, 2, "fif %d look-ahead %s" % (fif, lookahead))
            t = T.truth(samples, 2)
            assert np.array_equal(bits(p.ReadNoise()), bits(t["e"]))
            if lookahead:
                for _ in range(18):
                    p.Trace(True, 1)
            else:
                p.Trace(True, 18)
            got = (p.ReadNoiseMoments(), p.GetNoise(), p.ReadNoise(), p.ReadResult())
            assert got[1]["spp"] == 20
            if ref is None:
                ref = got
            else:
                tag = "fif %d look-ahead %s" % (fif, lookahead)
                assert np.array_equal(bits(got[0]), bits(ref[0])), tag
                assert got[1] == ref[1], tag
                assert np.array_equal(bits(got[2]), bits(ref[2])) and np.array_equal(bits(got[3]), bits(ref[3])), tag
            p.destroy()


@pytest.mark.parametrize("fif,lookahead", [(128, False), (5, True), (1, False)])
def test_trace_until(fif, lookahead, scene_cache, sobol_matrices):
    name, w, h, life, sub, spp = UNTIL
    inst, _ = _instance(scene_cache, UNTIL)
    p = inst.m_path_tracer
    samples, images = _truth(inst, UNTIL, sobol_matrices)
    every = 8
    wb = {n: T.truth(samples, n)["worst_block"] for n in range(every, spp + 1, every)}
    print("worst_block at the checkpoints:", {n: round(v, 4) for n, v in wb.items()})
    target = (wb[16] * wb[24]) ** 0.5
    assert wb[8] > target * (1 + 4 * REL) and wb[16] > target * (1 + 4 * REL) and wb[24] < target * (1 - 4 * REL)  # (chosen far from every checkpoint)
    p.SetFramesInFlight(fif)
    p.SetLookahead(lookahead)
    # statistics off: E_STATE
    with pytest.raises(N.AdyptError) as e:
        p.TraceUntil(target, 8, 64, every)
    assert e.value.code == N.E_STATE and p.GetSPP() == 0
    p.SetNoiseStats(True)
    for bad in ((target, 8, 64, 0), (target, 1, 64, 8), (target, 16, 8, 8), (target, 0, 0, 8)):
        with pytest.raises(N.AdyptError) as e:
            p.TraceUntil(*bad)
        assert e.value.code == N.E_INVALID and p.GetSPP() == 0
    g = p.TraceUntil(target, 8, 64, every)
    assert p.GetSPP() == 24 and g["spp"] == 24 and abs(g["worst_block"] - wb[24]) <= REL * wb[24] and g["worst_block"] <= target
    assert np.array_equal(bits(p.ReadResult()), bits(images[23])), "the image is not the plain trace's to 24 spp"
    _assert_moments(p, samples, 24)
    # a second call with a lower target continues the same accumulation: checkpoints 32, 40, 48
    target2 = (wb[40] * wb[48]) ** 0.5
    assert min(wb[32], wb[40]) > target2 * (1 + 4 * REL) and wb[48] < target2 * (1 - 4 * REL)
    g = p.TraceUntil(target2, 8, 64, every)
    assert p.GetSPP() == 48 and g["spp"] == 48 and g["worst_block"] <= target2
    assert np.array_equal(bits(p.ReadResult()), bits(images[47]))
    _assert_moments(p, samples, 48)
    # target 0: the cap is reached
    g = p.TraceUntil(0.0, 8, 64, every)
    assert p.GetSPP() == 64 and g["spp"] == 64 and g["worst_block"] > 0.0
    assert np.array_equal(bits(p.ReadResult()), bits(images[63]))
    g2 = p.TraceUntil(0.0, 8, 64, every)  # at the cap already: nothing is traced, the numbers are the same
    assert p.GetSPP() == 64 and g2 == g
    # a huge target: min_spp is respected (checkpoints 8, 16: the first at or above min_spp = 12 is 16)
    p.Reset()
    g = p.TraceUntil(1e30, 12, 64, every)
    assert p.GetSPP() == 16 and g["spp"] == 16
    assert np.array_equal(bits(p.ReadResult()), bits(images[15]))
    _assert_moments(p, samples, 16)
    p.destroy()


def test_zero_variance_stops_at_min_spp(scene_cache):
    """tiny2 from its table camera has zero variance in every pixel: noise 0 at every spp, so any target >= 0 stops at min_spp."""
    spec = scenes.make_scene("tiny2", scene_cache, width=64, height=48, pt={"tmpLifetime": 4, "maxBounce": 4, "subpixel": 1})
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=SEED), api.InstanceConfig.last_error()
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    g = p.TraceUntil(0.0, 6, 40, 3)
    assert p.GetSPP() == 6 and g["mean_noise"] == 0.0 and g["worst_block"] == 0.0 and g["worst_index"] == 0 and g["pixels"] == 64 * 48
    assert not p.ReadNoise().any()
    p.destroy()


def test_state_rules(scene_cache, sobol_matrices):
    case = CASES[1]
    name, w, h, life, sub, spp = case
    inst, _ = _instance(scene_cache, case)
    p = inst.m_path_tracer
    samples, images = _truth(inst, case, sobol_matrices)
    # off: every read-out says so
    for call in (p.GetNoise, p.ReadNoise, p.ReadNoiseMoments, p.ReadBlockNoise):
        with pytest.raises(N.AdyptError) as e:
            call()
        assert e.value.code == N.E_STATE
    p.Trace(True, 2)
    with pytest.raises(N.AdyptError) as e:
        p.SetNoiseStats(True)  # the moments start with the image
    assert e.value.code == N.E_STATE and not p.GetNoiseStats()
    p.SetNoiseStats(False)  # (disabling is always allowed)
    p.Reset()
    p.SetNoiseStats(True)
    assert not p.ReadNoiseMoments().any()  # nothing accumulated
    with pytest.raises(N.AdyptError) as e:
        p.GetNoise()
    assert e.value.code == N.E_STATE
    p.Trace(True, 1)
    with pytest.raises(N.AdyptError) as e:
        p.GetNoise()  # one frame has no variance estimate
    assert e.value.code == N.E_STATE
    _assert_moments(p, samples, 1)
    p.Trace(True, 4)
    first = (p.ReadNoiseMoments(), p.GetNoise(), p.ReadNoise())
    _assert_moments(p, samples, 5)
    # Reset() then tracing restarts the moments
    p.Reset()
    p.Trace(True, 3)
    _assert_moments(p, samples, 3, "after Reset")
    # Trace(False) then path tracing restarts them
    p.Trace(False)
    p.Trace(True, 7)
    _assert_moments(p, samples, 7, "after a viewer frame")
    assert np.array_equal(bits(p.ReadResult()), bits(images[6]))
    # a camera change without reset keeps them, like the image (same camera again: the same samples go on)
    ip, iv = inst.m_camera.matrices()
    p.SetCamera(ip, iv, inst.m_camera.position)
    p.Trace(True, 2)
    _assert_moments(p, samples, 9, "after SetCamera")
    # Reset, disable, enable, trace again: the same numbers again
    p.Reset()
    p.SetNoiseStats(False)
    assert not p.GetNoiseStats()
    p.SetNoiseStats(True)
    p.Trace(True, 5)
    again = (p.ReadNoiseMoments(), p.GetNoise(), p.ReadNoise())
    assert np.array_equal(bits(again[0]), bits(first[0])) and again[1] == first[1] and np.array_equal(bits(again[2]), bits(first[2]))
    # disabled in the middle of an accumulation: the image goes on as if nothing had been
    p.SetNoiseStats(False)
    p.Trace(True, 3)
    assert np.array_equal(bits(p.ReadResult()), bits(images[7]))
    p.destroy()


@pytest.mark.parametrize("case,n_dev", [(CASES[0], 3), (("tiny0", 64, 36, 4, 1, 12), 4), (("tiny0", 64, 36, 4, 1, 12), 1)],
                         ids=["100x75-3-shards", "64x36-4-shards-one-owns-nothing", "64x36-one-device"])  # (one device: what the CLI's --noise rests on)
def test_multi_device_on_one_card(case, n_dev, scene_cache, sobol_matrices, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    name, w, h, life, sub, spp = case
    inst, _ = _instance(scene_cache, case)
    single = inst.m_path_tracer
    c = inst.m_config
    m = api.MultiPathTracer()
    m.Initialize(c.pt_params(SEED), inst.m_hipscene, c.m_width, c.m_height, (0,) * n_dev)
    ip, iv = inst.m_camera.matrices()
    m.SetCamera(ip, iv, inst.m_camera.position)
    assert m.DeviceCount() == n_dev
    single.SetNoiseStats(True)
    m.SetNoiseStats(True)
    assert m.GetNoiseStats()
    single.Trace(True, spp)
    m.Trace(True, spp)
    samples, images = _truth(inst, case, sobol_matrices)
    _assert_moments(single, samples, spp)
    assert np.array_equal(bits(m.ReadNoiseMoments()), bits(single.ReadNoiseMoments()))
    gs, gm = single.GetNoise(), m.GetNoise()
    assert gm == gs and gm["pixels"] == w * h
    assert np.array_equal(bits(m.ReadNoise()), bits(single.ReadNoise()))
    a, b = m.ReadBlockNoise(), single.ReadBlockNoise()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and np.array_equal(a[2], b[2])
    assert np.array_equal(bits(m.ReadResult()), bits(images[spp - 1]))
    # TraceUntil stops at the same spp
    single.Reset()
    m.Reset()
    t2, t4, t6 = (T.truth(samples, n)["worst_block"] for n in (2, 4, 6))
    target = (t4 * t6) ** 0.5
    assert t2 > target * (1 + 4 * REL) and t4 > target * (1 + 4 * REL) and t6 < target * (1 - 4 * REL)
    gs, gm = single.TraceUntil(target, 2, spp, 2), m.TraceUntil(target, 2, spp, 2)
    assert single.GetSPP() == 6 and m.GetSPP() == 6 and gm == gs
    assert np.array_equal(bits(m.ReadResult()), bits(images[5]))
    m.destroy()
    single.destroy()


# the loop and the bound of tests/test_gpu_memory.py: its measured drift (0) plus one 2 MiB granule of the runtime's allocator
BOUND_BYTES = 0 + (2 << 20)


def _free_bytes():
    free = api.device_free_bytes(0)
    if free is None:
        import torch
        free = torch.cuda.mem_get_info(0)[0]
    return int(free)


def test_enabling_and_disabling_gives_the_memory_back(scene_cache):
    """One context; ten cycles of enable, trace, query, disable.  At 1024 x 768 the moments alone are 768 blocks x 1024 x 8 B = 6 MiB: one set
    forgotten in one cycle is three times the bound."""
    spec = scenes.make_scene("tiny0", scene_cache, width=1024, height=768, pt={"maxBounce": 4, "stackSize": 16})
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=7), api.InstanceConfig.last_error()
    p = inst.m_path_tracer
    p.SetFramesInFlight(4)
    a = _free_bytes()
    time.sleep(1.0)
    b = _free_bytes()
    if abs(a - b) > BOUND_BYTES:
        pytest.skip("another process is changing the device's free memory (%d bytes within a second)" % abs(a - b))
    after = {}
    for cycle in range(1, 11):
        p.Reset()
        p.SetNoiseStats(True)
        p.Trace(True, 3)
        p.GetNoise(); p.ReadNoise(); p.ReadNoiseMoments(); p.ReadBlockNoise()
        p.TraceUntil(0.0, 2, 5, 2)
        if cycle == 5:
            during = _free_bytes()
        p.SetNoiseStats(False)
        after[cycle] = _free_bytes()
    print("free bytes after each cycle:", after, "| drift 2 -> 10:", after[2] - after[10], "| held while on:", after[5] - during)
    assert after[5] - during >= 768 * 1024 * 8, "the statistics' buffers were not there while the feature was on"
    assert abs(after[2] - after[10]) <= BOUND_BYTES, after
    p.destroy()


def test_cli_renders_to_a_noise_target(scene_cache, sobol_matrices, tmp_path):
    name, w, h, life, sub, spp = UNTIL
    inst, spec = _instance(scene_cache, UNTIL)
    samples, images = _truth(inst, UNTIL, sobol_matrices)
    wb = {n: T.truth(samples, n)["worst_block"] for n in (8, 16, 24, 32)}
    target = (wb[24] * wb[32]) ** 0.5
    assert min(wb[8], wb[16], wb[24]) > target * (1 + 4 * REL) and wb[32] < target * (1 - 4 * REL)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    g = p.TraceUntil(target, 8, 64, 8)
    assert p.GetSPP() == 32
    img, e = p.ReadResult(), p.ReadNoise()
    p.destroy()
    a_exr, n_exr = str(tmp_path / "a.exr"), str(tmp_path / "n.exr")
    r = subprocess.run([CLI, spec.config_path, "--noise", repr(target), "--spp", "64", "--check-every", "8", "--min-spp", "8", "--out", a_exr, "--noise-out", n_exr,
                        "--seed", str(SEED)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    text = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, text[-2000:]
    line = re.search(r"\[PT\]NOISE: spp (\d+) mean_noise (\S+) worst_block (\S+) worst_index (-?\d+)", text)
    assert line, text[-2000:]
    assert int(line.group(1)) == 32 and int(line.group(4)) == g["worst_index"]
    assert float(line.group(2)) == float("%.9g" % g["mean_noise"]) and float(line.group(3)) == float("%.9g" % g["worst_block"])
    assert np.array_equal(bits(api.load_exr(a_exr)), bits(img)) and np.array_equal(bits(img), bits(images[31]))
    grey = api.load_exr(n_exr)
    for ch in range(3):
        assert np.array_equal(bits(grey[..., ch]), bits(e))
    # without --noise the CLI is what it was: a fixed count, no noise line
    r = subprocess.run([CLI, spec.config_path, "--spp", "32", "--out", a_exr, "--seed", str(SEED)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0 and b"NOISE" not in r.stdout
    assert np.array_equal(bits(api.load_exr(a_exr)), bits(img))
