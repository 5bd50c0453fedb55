"""-m gpu: the temporal merge through mirrors and glass by the virtual point (include/adypt_hip.h adypt_denoise_temporal_specular ...; guide_chain.hpp,
temporal.hpp; k_chain_start<true>, k_chain_step<true>, k_denoise_prepare_virtual, k_temporal_merge_virtual in denoise_kernels.hpp).  The truth is computed
in this process by the numpy restatement (tests/virtual_truth.py) from what the CPU ORACLE gives for every pose — its image, the moments of its samples,
its primary frames, its closest hits for every bounce — never from the library's read-outs; the truth's history is the truth's own.  Bit for bit."""
import inspect

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import denoise_truth as D  # noqa: E402
from tests import specular_truth as S  # noqa: E402
from tests import temporal_truth as TT  # noqa: E402
from tests import test_gpu_denoise as GD  # noqa: E402           (its state read-outs)
from tests import test_gpu_denoise_specular as GS  # noqa: E402  (its comparison of the chain's guides and counts)
from tests import test_gpu_denoise_temporal as GT  # noqa: E402  (its cameras a step apart)
from tests import test_gpu_noise as G  # noqa: E402
from tests import virtual_scenes as VS  # noqa: E402
from tests import virtual_truth as V  # noqa: E402
from tests.helpers import bits, oracle_scene_from_instance  # noqa: E402

F = np.float32
SEED, SPP = 31, 4
TINY0 = G.CASES[0]  # tiny0 100x75: partial blocks on two edges; escaped, truncated and multi-bounce chains
HAS_FEATURE = "follow_specular" in inspect.signature(api.HipPathTracer.Denoise).parameters
_poses = {}


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def tiny0_pose(inst, k, sobol_matrices, spp=SPP):
    """(position, yaw, seed, the oracle's pose) of tiny0's camera k steps on, once"""
    c = inst.m_config.c
    pos, yaw = GT.camera_of(c, "tiny0", k)
    key = ("tiny0", c.width, c.height, k, spp)
    if key not in _poses:
        osc = oracle_scene_from_instance(inst)
        ip, iv = O.camera(c.fov, yaw, c.pitch, c.width, c.height)
        P = O.make_params(c.width, c.height, pos, ip, iv, stack_size=c.stack_size, max_bounce=c.max_bounce, subpixel=c.subpixel, tmp_life=c.tmp_lifetime, tmin=c.ray_tmin,
                          clamp=c.clamp, sun=list(c.sun))
        pose = VS.oracle_pose(osc, P, SEED + k, sobol_matrices, spp, frames=spp + 2)
        pose.update(osc=osc, P=P, cam=(np.array(pos, np.float32), ip, iv))
        _poses[key] = pose
    return pos, yaw, SEED + k, _poses[key]


def guides(pose, K):
    key = ("guides", K)
    if key not in pose:
        pose[key] = V.chain_guides(pose["osc"], pose["P"], K, pose["primary"])
    return pose[key]


def truth(pose, K, hist, **kw):
    return V.denoise(pose["image"], pose["m2"], pose["spp"], guides(pose, K), hist, pose["cam"], K, **kw)


def plain_call(pose):
    g = pose["primary"]
    return (pose["image"], pose["m2"], pose["spp"], g["albedo"], g["normal"], g["position"], g["tri"] != -1)


def assert_call(p, want, g, K, tag):
    """what a followed call left behind, read back: the history length, the virtual points, the counts of the merge and of the chain"""
    out, n_out, _, counts = want
    assert same(p.ReadDenoiseHistory(), n_out), tag + ": the history length"
    v = p.ReadDenoiseVirtual()
    assert same(v["virtual_position"], g["virtual"]), "%s: %d words of the virtual points differ" % (tag, int((bits(v["virtual_position"]) != bits(g["virtual"])).sum()))
    assert same(v["distance"], g["distance"]), tag + ": the unfolded lengths"
    info = p.GetDenoiseVirtual()
    assert info["have"] == 1 and info["bounces"] == K and info["device_bytes"] > 0, (tag, info)
    assert (info["pixels_followed"], info["pixels_with_history"]) == (counts["followed"], counts["with_history"]), (tag, info, counts)
    GS.assert_counts(p.GetDenoiseSpecular(), g, K, tag)
    assert p.GetDenoiseMergeMs() > 0.0


@pytest.mark.parametrize("K", [2, 8])
def test_tiny0_two_poses(K, scene_cache, sobol_matrices):
    inst, _ = G._instance(scene_cache, TINY0)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    assert p.GetDenoiseVirtual()["have"] == 0
    hist = None
    for k in (0, 1):
        pos, yaw, seed, pose = tiny0_pose(inst, k, sobol_matrices)
        g = guides(pose, K)
        c = g["chain"]
        assert (c < 0).any() and (c >= 2).any() and (c == 0).any() and (c == 1).any() and (K == 8 or g["truncated"] > 0)
        GT.set_pose(p, inst.m_config, pos, yaw, seed)
        assert same(p.ReadResult(), pose["image"]), "camera %d: the image is not the oracle's" % k
        before, hits_before = GD.state_of(p), p.ReadHits()
        want = truth(pose, K, hist)
        if k == 1:  # the history is only read: two calls leave the same bits
            a, na = p.Denoise(temporal=True, follow_specular=K, commit=False), p.ReadDenoiseHistory()
            b, nb = p.Denoise(temporal=True, follow_specular=K, commit=False), p.ReadDenoiseHistory()
            assert same(a, want[0]) and same(b, want[0]) and same(na, want[1]) and same(nb, want[1]), "commit=False"
            assert want[3]["with_history"] > 0 and (want[1][c == 1] > F(SPP)).mean() > 0.5, "the case merges next to nothing"
        got = p.Denoise(temporal=True, follow_specular=K)
        assert same(got, want[0]), "camera %d: %d words of the result differ" % (k, int((bits(got) != bits(want[0])).sum()))
        assert_call(p, want, g, K, "camera %d K = %d" % (k, K))
        if k == 0:
            assert (want[1] == F(SPP)).all() and same(got, S.denoise(pose["image"], pose["m2"], SPP, g["albedo"], g["normal"], g["position"], c)), "the first call is the followed filter"
        GS.assert_chain(p.ReadDenoiseGuides(specular_bounces=K), g, "the guides the call filtered with, camera %d" % k)
        GD.assert_same_state(GD.state_of(p), before, "around the followed calls at camera %d" % k)
        hits_after = p.ReadHits()
        assert np.array_equal(hits_after[0], hits_before[0]) and same(hits_after[1], hits_before[1]), "the primary-hit cache moved"
        hist = want[2]
    p.Trace(True, 2)
    assert p.GetSPP() == SPP + 2 and same(p.ReadResult(), pose["images"][SPP + 1]), "tracing on afterwards left the oracle's image"
    p.destroy()


def test_planar_scene_and_its_derived_lengths(sobol_matrices):
    """45 x 21: neither a multiple of 32 wide nor of 8 high.  2 spp per pose: every pixel whose virtual point reprojects inside the history has four
    taps of the same wall, each of length 2, and n_out == 4 exactly (tests/test_virtual_definition.py derives it) — here read back from the device."""
    b = VS.Planar(45, 21)
    p = b.tracer()
    p.SetNoiseStats(True)
    for K in (1, 8):
        p.ResetDenoiseHistory()
        hist = None
        for k in (0, 1):
            key = ("planar", k)
            if key not in _poses:
                osc, P = b.oracle_at(k)
                _poses[key] = VS.oracle_pose(osc, P, SEED + k, sobol_matrices, 2)
                _poses[key].update(osc=osc, P=P, cam=b.camera(k))
            pose = _poses[key]
            g = guides(pose, K)
            pos, ip, iv = b.camera(k)
            p.Reset()
            p.SetConfig(b.pt_params(SEED + k))
            p.SetCamera(ip, iv, pos)
            p.Trace(True, 2)
            assert same(p.ReadResult(), pose["image"]), "camera %d: the image is not the oracle's" % k
            want = truth(pose, K, hist)
            got = p.Denoise(temporal=True, follow_specular=K)
            assert same(got, want[0]), "planar camera %d K = %d" % (k, K)
            assert_call(p, want, g, K, "planar camera %d K = %d" % (k, K))
            if k == 1:
                ok, fx, fy, _ = TT.reproject(hist["cam"], 45, 21, g["virtual"])
                inside = ok & (fx >= 0) & (fx <= F(44)) & (fy >= 0) & (fy <= F(20))
                n_out = p.ReadDenoiseHistory()
                assert inside.sum() > 45 * 21 // 2 and (n_out[inside] == F(4)).all()
                assert p.GetDenoiseVirtual()["pixels_followed"] == 45 * 21
            hist = want[2]
    p.destroy()


def test_history_kinds(scene_cache, sobol_matrices):
    """a followed call finds no history of another kind or another K, the plain temporal call none in a followed call's; ResetDenoiseHistory() drops it"""
    inst, _ = G._instance(scene_cache, TINY0)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    pos, yaw, seed, pose = tiny0_pose(inst, 1, sobol_matrices)
    GT.set_pose(p, inst.m_config, pos, yaw, seed)
    call = plain_call(pose)
    none8, none2, plain_none = truth(pose, 8, None), truth(pose, 2, None), TT.denoise(*call, None, pose["cam"])
    assert same(p.Denoise(temporal=True, follow_specular=8), none8[0])
    # in a followed history of 8 bounces: the plain call and another K find none, the same K finds it
    got, n = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
    assert same(got, plain_none[0]) and same(n, plain_none[1]) and (n == F(SPP)).all(), "the plain temporal call found a followed history"
    got, n = p.Denoise(temporal=True, follow_specular=2, commit=False), p.ReadDenoiseHistory()
    assert same(got, none2[0]) and same(n, none2[1]), "K = 2 found the history of K = 8"
    own = truth(pose, 8, none8[2])
    got, n = p.Denoise(temporal=True, follow_specular=8, commit=False), p.ReadDenoiseHistory()
    assert same(got, own[0]) and same(n, own[1]) and not same(own[0], none8[0]) and own[3]["with_history"] > 0
    assert p.GetDenoiseVirtual()["pixels_with_history"] == own[3]["with_history"]
    # the other way round: the plain call commits, the followed call finds none; and the plain call finds its own
    assert same(p.Denoise(temporal=True), plain_none[0])
    got, n = p.Denoise(temporal=True, follow_specular=8, commit=False), p.ReadDenoiseHistory()
    assert same(got, none8[0]) and same(n, none8[1]), "the followed call found a plain history"
    want = TT.denoise(*call, plain_none[2], pose["cam"])
    assert same(p.Denoise(temporal=True, commit=False), want[0])
    # a followed commit replaces it; ResetDenoiseHistory() drops it
    assert same(p.Denoise(temporal=True, follow_specular=8), none8[0])
    assert same(p.Denoise(temporal=True, follow_specular=8, commit=False), own[0])
    p.ResetDenoiseHistory()
    got, n = p.Denoise(temporal=True, follow_specular=8, commit=False), p.ReadDenoiseHistory()
    assert same(got, none8[0]) and (n == F(SPP)).all()
    p.destroy()


def test_existing_calls_are_what_they_were(scene_cache, sobol_matrices):
    """after followed temporal calls on the same context (where the library has them) Denoise(), Denoise(specular_bounces=K), Denoise(temporal=True) and the
    guide read-outs give their own truths' bits"""
    inst, _ = G._instance(scene_cache, TINY0)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    pos, yaw, seed, pose = tiny0_pose(inst, 0, sobol_matrices)
    GT.set_pose(p, inst.m_config, pos, yaw, seed)
    if HAS_FEATURE:
        p.Denoise(temporal=True, follow_specular=8)
        p.Denoise(temporal=True, follow_specular=3, commit=False)
    call = plain_call(pose)
    assert same(p.Denoise(), D.denoise(*call)), "Denoise()"
    for K in (2, 8):
        g = guides(pose, K)
        assert same(p.Denoise(specular_bounces=K), S.denoise(pose["image"], pose["m2"], SPP, g["albedo"], g["normal"], g["position"], g["chain"])), "Denoise(specular_bounces=%d)" % K
        GS.assert_chain(p.ReadDenoiseGuides(specular_bounces=K), g, "K = %d" % K)
        GS.assert_counts(p.GetDenoiseSpecular(), g, K, "K = %d" % K)
    p.ResetDenoiseHistory()
    first = TT.denoise(*call, None, pose["cam"])
    assert same(p.Denoise(temporal=True), first[0])
    second = TT.denoise(*call, first[2], pose["cam"])
    assert same(p.Denoise(temporal=True, commit=False), second[0]) and same(p.ReadDenoiseHistory(), second[1])
    got = p.ReadDenoiseGuides()
    for k in ("albedo", "normal", "position"):
        assert same(got[k], pose["primary"][k]), k
    assert np.array_equal(got["hit"], pose["primary"]["tri"] != -1)
    p.destroy()


@pytest.mark.parametrize("n_dev", [2, 3])
def test_multi_device_on_one_card(n_dev, scene_cache, sobol_matrices, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    inst, _ = G._instance(scene_cache, TINY0)
    single, c = inst.m_path_tracer, inst.m_config
    m = api.MultiPathTracer()
    m.Initialize(c.pt_params(SEED), inst.m_hipscene, c.m_width, c.m_height, (0,) * n_dev)
    assert m.DeviceCount() == n_dev
    K, hist = 4, None
    for t in (single, m):
        t.SetNoiseStats(True)
    for k in (0, 1):
        pos, yaw, seed, pose = tiny0_pose(inst, k, sobol_matrices)
        g = guides(pose, K)
        want = truth(pose, K, hist)
        for t in (single, m):
            GT.set_pose(t, c, pos, yaw, seed)
        a, b = single.Denoise(temporal=True, follow_specular=K), m.Denoise(temporal=True, follow_specular=K)
        assert same(a, want[0]) and same(b, a), "%d shards against one context, camera %d" % (n_dev, k)
        assert_call(m, want, g, K, "%d shards, camera %d" % (n_dev, k))
        hist = want[2]
    assert want[3]["with_history"] > 0
    sp = N.SpecularParams(K)  # a shard context refuses the per-context call
    with pytest.raises(N.AdyptError) as e:
        N.check(N.lib.adypt_denoise_temporal_specular(m._contexts()[0], None, None, N.C.byref(sp)), m._contexts()[0])
    assert e.value.code == N.E_STATE and "tile shard" in str(e.value)
    m.destroy()
    single.destroy()


def test_refusals_leave_the_history_and_the_result(scene_cache, sobol_matrices):
    inst, _ = G._instance(scene_cache, TINY0)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    ctx = p._ctx
    out = N.DenoiseVirtual()
    assert N.lib.adypt_read_denoise_virtual(ctx, None, None) == N.E_STATE and N.lib.adypt_get_denoise_virtual(ctx, None) == N.E_INVALID
    assert N.lib.adypt_get_denoise_virtual(ctx, N.C.byref(out)) == N.ADYPT_OK and out.have == 0
    pos, yaw, seed, pose = tiny0_pose(inst, 0, sobol_matrices)
    GT.set_pose(p, inst.m_config, pos, yaw, seed)
    p.Denoise(temporal=True, follow_specular=2)
    last, n_last = p.Denoise(temporal=True, follow_specular=2, commit=False), p.ReadDenoiseHistory()
    assert (n_last > F(SPP)).any()

    def untouched(tag):
        rgb = np.zeros_like(last)
        N.check(N.lib.adypt_read_denoised(ctx, rgb.ctypes.data), ctx)
        assert same(rgb, last) and same(p.ReadDenoiseHistory(), n_last), tag + ": the last result moved"

    tp = N.TemporalParams(64.0, 1)
    for bad in (0, 9, -1):
        sp = N.SpecularParams(bad)
        assert N.lib.adypt_denoise_temporal_specular(ctx, None, N.C.byref(tp), N.C.byref(sp)) == N.E_INVALID and b"bounces must be in [1, 8]" in N.lib.adypt_last_error(ctx)
        untouched("bounces %d" % bad)
    sp = N.SpecularParams(2)
    assert N.lib.adypt_denoise_temporal_specular(ctx, None, N.C.byref(tp), None) == N.E_INVALID and b"specular is null" in N.lib.adypt_last_error(ctx)
    bad_levels = N.DenoiseParams(0, 4.0, 0.1)
    assert N.lib.adypt_denoise_temporal_specular(ctx, N.C.byref(bad_levels), N.C.byref(tp), N.C.byref(sp)) == N.E_INVALID
    for cap in (0.0, -1.0, float("nan"), float("inf")):
        bad_cap = N.TemporalParams(cap, 1)
        assert N.lib.adypt_denoise_temporal_specular(ctx, None, N.C.byref(bad_cap), N.C.byref(sp)) == N.E_INVALID and b"history_cap" in N.lib.adypt_last_error(ctx)
    untouched("the C refusals")
    for kw in (dict(follow_specular=2), dict(temporal=True, follow_specular=9), dict(temporal=True, follow_specular=-1), dict(temporal=True, follow_specular=2, specular_bounces=2),
               dict(temporal=True, follow_specular=2, follow_motion=True), dict(temporal=True, follow_specular=2, rectify=True), dict(temporal=True, follow_specular=2, moments=True),
               dict(temporal=True, specular_bounces=2)):
        with pytest.raises(ValueError):
            p.Denoise(**kw)
    untouched("the Python refusals")
    # the history is as it was: the same call gives the same bits
    assert same(p.Denoise(temporal=True, follow_specular=2, commit=False), last) and same(p.ReadDenoiseHistory(), n_last)
    p.Trace(False)
    with pytest.raises(N.AdyptError) as e:
        p.Denoise(temporal=True, follow_specular=2)
    assert e.value.code == N.E_STATE and "not path-traced" in str(e.value)
    p.destroy()


def test_cli(scene_cache, tmp_path):
    """--follow-specular K makes every temporal call a followed one, the --history-from pose included: the files are the library's bits"""
    import os
    import re
    import subprocess
    name, w, h, life, sub, _ = TINY0
    inst, spec = G._instance(scene_cache, TINY0)
    p, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    p.SetNoiseStats(True)
    K, spp = 4, SPP
    pos, yaw = [float(v) for v in c.position], c.yaw
    GT.set_pose(p, cfg, pos, yaw, SEED + 1, spp)  # the history pose: the same config, the seed the command line gives it
    p.Denoise(temporal=True, follow_specular=K)
    GT.set_pose(p, cfg, pos, yaw, SEED, spp)
    den, n_out, g, info = p.Denoise(temporal=True, follow_specular=K), p.ReadDenoiseHistory(), p.ReadDenoiseGuides(specular_bounces=K), p.GetDenoiseVirtual()
    p.destroy()
    assert info["pixels_followed"] > 0 and info["pixels_with_history"] > 0
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    out, d_exr, h_exr, prefix = str(tmp_path / "o.exr"), str(tmp_path / "d.exr"), str(tmp_path / "h.exr"), str(tmp_path / "g")
    r = subprocess.run([exe, spec.config_path, "--out", out, "--seed", str(SEED), "--spp", str(spp), "--denoise", d_exr, "--history-from", spec.config_path, "--history-out", h_exr,
                        "--follow-specular", str(K), "--guides-out", prefix], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "Saved denoised image (5 levels)" in text, text[-2000:]
    assert same(api.load_exr(d_exr), den), "the denoised image"
    assert same(api.load_exr(h_exr)[..., 0], n_out), "the history lengths"
    for k in ("albedo", "normal", "position"):
        assert same(api.load_exr("%s.%s.exr" % (prefix, k)), g[k]), k
    assert np.array_equal(api.load_exr(prefix + ".chain.exr")[..., 0], g["chain"].astype(np.float32)), "chain classes"
    m = re.search(r"\[PT\]TEMPORAL: history on \d+ of \d+ hit pixels, mean length [0-9.]+, followed (\d+) pixels, (\d+) with history\n", text)
    assert m, text[-2000:]
    assert [int(v) for v in m.groups()] == [info["pixels_followed"], info["pixels_with_history"]], (m.groups(), info)
