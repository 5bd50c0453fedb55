"""-m gpu: guides that follow mirrors and glass (include/adypt_hip.h adypt_denoise_specular ...; csrc/device/guide_chain.hpp, denoise.hip).  The truth is
computed in this process by the numpy restatement (tests/specular_truth.py) from what the CPU ORACLE gives — its primary frames, its closest hits for
every bounce, its image and the moments of its samples — never from the library's read-outs; everything is compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import noise_truth as T  # noqa: E402
from tests import specular_scenes as SC  # noqa: E402
from tests import specular_truth as S  # noqa: E402
from tests import test_gpu_adaptive as A  # noqa: E402
from tests import test_gpu_denoise as GD  # noqa: E402  (its state read-outs and its truth's inputs)
from tests import test_gpu_noise as G  # noqa: E402
from tests.helpers import bits, oracle_scene_from_instance  # noqa: E402
from tests.test_gpu_parity import make_instance  # noqa: E402

SEED = G.SEED
TINY0, SIBENIK = G.CASES[0], G.CASES[2]  # tiny0 100x75 (partial blocks on two edges), sibenik 160x90
_chains = {}


def chains_of(inst, case, K):
    key = case[:5] + (K,)
    if key not in _chains:
        osc, P = oracle_scene_from_instance(inst), T.oracle_params(inst.m_config.c)
        pk = case[:5] + ("primary",)
        if pk not in _chains:
            _chains[pk] = S.primary_guides(osc, P)
        g = S.chain_guides(osc, P, K, _chains[pk])
        for v in g.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _chains[key] = g
    return _chains[key]


def assert_chain(got, want, tag=""):
    for k in ("albedo", "normal", "position"):
        differing = int((bits(got[k]) != bits(want[k])).sum())
        assert differing == 0, "%s: %d words of %s differ %s" % (k, differing, k, tag)
    assert got["chain"].dtype == np.int8 and np.array_equal(got["chain"], want["chain"]), "chain " + tag
    assert np.array_equal(got["hit"], want["hit"]), "hit " + tag


def assert_counts(info, want, K, tag=""):
    assert info["have"] == 1 and info["bounces"] == K and info["chain_ms"] > 0.0 and info["device_bytes"] > 0, tag
    for k, name in (("rays", "rays"), ("pixels_followed", "followed"), ("pixels_escaped", "escaped"), ("pixels_truncated", "truncated")):
        assert info[k] == want[name], "%s: %s %d, the truth %d" % (tag, k, info[k], want[name])


def filter_truth(inst, case, samples, images, n, g, **kw):
    image, m2 = images[n - 1], T.moments(samples[:n])[1]
    return S.denoise(image, m2, n, g["albedo"], g["normal"], g["position"], g["chain"], **kw)


def run_case(case, Ks, scene_cache, sobol_matrices):
    name, w, h, life, sub, spp = case
    inst, _ = G._instance(scene_cache, case)
    p = inst.m_path_tracer
    samples, images = G._truth(inst, case, sobol_matrices)
    p.SetNoiseStats(True)
    mid = life + 1 if life + 1 < spp else 5  # in the middle of a tmpLifetime group: a clobbered primary-hit cache or ray queue would show in the frames that follow
    assert mid % life != 0 and 2 <= mid < spp
    p.Trace(True, mid)
    before, hits_before = GD.state_of(p), p.ReadHits()
    for K in Ks:
        g = chains_of(inst, case, K)
        got = p.Denoise(specular_bounces=K)
        assert np.array_equal(bits(got), bits(filter_truth(inst, case, samples, images, mid, g))), "Denoise(specular_bounces=%d) at %d spp" % (K, mid)
        assert_counts(p.GetDenoiseSpecular(), g, K, "K = %d" % K)
        assert_chain(p.ReadDenoiseGuides(specular_bounces=K), g, "K = %d" % K)
        assert_counts(p.GetDenoiseSpecular(), g, K, "K = %d, after the guide read-out" % K)
    GD.assert_guides(p.ReadDenoiseGuides(), GD.guides_of(inst, case), "the plain guides after the followed ones")
    assert np.array_equal(bits(p.Denoise()), bits(GD.truth(inst, case, samples, images, mid))), "plain Denoise() after the followed ones"
    GD.assert_same_state(GD.state_of(p), before, "around the specular calls")
    hits_after = p.ReadHits()
    assert np.array_equal(hits_after[0], hits_before[0]) and np.array_equal(bits(hits_after[1]), bits(hits_before[1])), "the primary-hit cache moved"
    p.Trace(True, spp - mid)
    assert p.GetSPP() == spp and np.array_equal(bits(p.ReadResult()), bits(images[spp - 1])), "tracing on afterwards left the oracle's image"
    G._assert_moments(p, samples, spp, "after the specular calls")
    p.destroy()


def test_tiny0_guides_filter_and_state(scene_cache, sobol_matrices):
    inst, _ = G._instance(scene_cache, TINY0)
    c = chains_of(inst, TINY0, 8)["chain"]
    assert (c < 0).any(), "an escaped pixel"
    assert (c == 2).any(), "one bounce"
    assert (c >= 4).any() or (c <= -4).any(), "three bounces or more"
    osc = oracle_scene_from_instance(inst)
    glass = np.isin(osc.materials["illum"][osc.triangles["matid"][np.maximum(_chains[TINY0[:5] + ("primary",)]["tri"], 0)]], (6, 7)) & (c != 0)
    assert (glass & ((c >= 3) | (c <= -3))).any(), "a pixel through two glass interfaces"
    for K in (1, 2):
        assert chains_of(inst, TINY0, K)["truncated"] > 0, "a truncated pixel at K = %d" % K
    inst.m_path_tracer.destroy()
    run_case(TINY0, (1, 2, 8), scene_cache, sobol_matrices)


def test_sibenik(scene_cache, sobol_matrices):
    run_case(SIBENIK, (4,), scene_cache, sobol_matrices)


def test_without_delta_materials_it_is_the_plain_filter(scene_cache):
    inst = make_instance(scene_cache, "tiny0", 100, 75)
    mats = np.array(inst.scene.materials).view(O.MAT_DT).copy()
    assert np.isin(mats["illum"], (3, 4, 5, 6, 7)).any()
    mats["illum"][np.isin(mats["illum"], (3, 4, 5, 6, 7))] = 1
    sc = api.Scene.FromArrays(np.array(inst.scene.triangles), mats)
    sc.textures = inst.scene.textures
    hs = api.HipScene()
    hs.Initialize(sc, inst.bvh)
    p = api.HipPathTracer()
    p.Initialize(inst.m_config.pt_params(SEED), hs, 100, 75)
    ip, iv = inst.m_camera.matrices()
    p.SetCamera(ip, iv, inst.m_camera.position)
    p.SetNoiseStats(True)
    p.Trace(True, 5)
    plain = p.Denoise()
    assert np.array_equal(bits(p.Denoise(specular_bounces=8)), bits(plain))
    info = p.GetDenoiseSpecular()
    assert info["rays"] == 0 and info["pixels_followed"] == 0 and info["have"] == 1
    g, f = p.ReadDenoiseGuides(), p.ReadDenoiseGuides(specular_bounces=8)
    for k in ("albedo", "normal", "position", "hit"):
        assert np.array_equal(g[k], f[k]), k
    assert np.array_equal(f["chain"], g["hit"].astype(np.int8))
    p.destroy()
    inst.m_path_tracer.destroy()


SHAPES = [(32, 18), (33, 33)]  # one block; four blocks, all partial


@pytest.mark.parametrize("shape", SHAPES, ids=["32x18", "33x33"])
@pytest.mark.parametrize("name", ["facing_mirrors", "mirror_under_sky", "glass_box", "mirror_shows_texture"])
def test_hand_made_scenes(name, shape, scene_cache):
    b = SC.Built(name, *shape)
    osc, P = b.oracle()
    p = b.tracer()
    n = shape[0] * shape[1]
    for K in (1, 3):
        g = S.chain_guides(osc, P, K)
        if name == "facing_mirrors":
            assert g["followed"] == n and g["truncated"] == n and g["rays"] == K * n and (g["chain"] == 1 + K).all()
        elif name == "mirror_under_sky":
            assert g["escaped"] == n and (g["chain"] == -1).all()
        elif name == "glass_box":
            assert g["escaped"] > 0 and (K == 1 or (g["chain"] <= -3).any()), "total internal reflection, then transmission"
        else:
            assert (g["chain"] == 2).all() and len(np.unique(g["albedo"].reshape(-1, 3), axis=0)) > n // 2, "the texture path"
        assert_chain(p.ReadDenoiseGuides(specular_bounces=K), g, "%s K = %d" % (name, K))
        assert_counts(p.GetDenoiseSpecular(), g, K, "%s K = %d" % (name, K))
    p.destroy()


@pytest.mark.parametrize("shape", [(8, 8), (16, 16), (96, 64)], ids=["one-wave", "one-workgroup", "several-workgroups-per-segment"])
def test_queue_thresholds(shape, scene_cache):
    """an all-mirror wall fills the view and every ray survives every round: the fullest queues a picture of that size can give"""
    b = SC.Built("facing_mirrors", *shape)
    osc, P = b.oracle()
    p = b.tracer()
    n = shape[0] * shape[1]
    g = S.chain_guides(osc, P, 3)
    assert g["rays"] == 3 * n
    assert_chain(p.ReadDenoiseGuides(specular_bounces=3), g)
    assert_counts(p.GetDenoiseSpecular(), g, 3)
    p.destroy()


def test_exactly_one_chain_pixel(scene_cache):
    b = SC.Built("one_chain_pixel", 32, 18)
    osc, P = b.oracle()
    g = S.chain_guides(osc, P, 2)
    assert g["followed"] == 1 and g["rays"] >= 1
    p = b.tracer()
    assert_chain(p.ReadDenoiseGuides(specular_bounces=2), g)
    assert_counts(p.GetDenoiseSpecular(), g, 2)
    p.destroy()


@pytest.mark.parametrize("shape,n_dev", [((100, 75), 2), ((100, 75), 3), ((64, 36), 4)], ids=["100x75-2", "100x75-3", "64x36-4-one-owns-nothing"])
def test_multi_device_on_one_card(shape, n_dev, scene_cache, sobol_matrices, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    w, h = shape
    case = ("tiny0", w, h, 16, 3, 9)
    inst, _ = G._instance(scene_cache, case)
    single = inst.m_path_tracer
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
    g = chains_of(inst, case, 4)
    a, b = single.Denoise(specular_bounces=4), m.Denoise(specular_bounces=4)
    assert np.array_equal(bits(a), bits(b)), "%d shards against one context" % n_dev
    assert_chain(m.ReadDenoiseGuides(specular_bounces=4), g, "%d shards" % n_dev)
    assert_counts(m.GetDenoiseSpecular(), g, 4, "%d shards" % n_dev)
    assert np.array_equal(bits(m.Denoise()), bits(single.Denoise())), "the plain filter afterwards"
    if n_dev > 1:  # a shard context refuses the per-context call
        sp = N.SpecularParams(4)
        with pytest.raises(N.AdyptError) as e:
            N.check(N.lib.adypt_denoise_specular(m._contexts()[0], None, N.C.byref(sp)), m._contexts()[0])
        assert e.value.code == N.E_STATE and "tile shard" in str(e.value)
    m.destroy()
    single.destroy()


def test_after_trace_adaptive_the_guides_cover_every_owned_block(scene_cache, sobol_matrices):
    case = A.TINY0
    name, w, h, life, sub, every, min_spp, cap, nominal = case
    inst, _ = A._instance(scene_cache, case)
    p = inst.m_path_tracer
    samples, images = A._truth(inst, case, sobol_matrices)
    table, target, spp_b, counter, frozen = A.plan_of(case, samples)
    spp32, counter32, frozen32 = A.schedule(table, target, every, min_spp, 32)
    assert 0 < len(frozen32) < len(spp32)
    p.SetNoiseStats(True)
    p.TraceAdaptive(target, min_spp, 32, every)
    g = chains_of(inst, case, 8)
    assert_chain(p.ReadDenoiseGuides(specular_bounces=8), g, "with blocks frozen")
    want = A.expected(samples, images, w, h, spp32)
    truth = S.denoise(want["image"], want["moments"][..., 1], spp32, g["albedo"], g["normal"], g["position"], g["chain"])
    assert np.array_equal(bits(p.Denoise(specular_bounces=8)), bits(truth)), "Denoise(specular_bounces=8) with blocks frozen"
    p.destroy()


def test_after_update_triangles_the_chain_follows_the_geometry(scene_cache):
    b = SC.Built("mirror_shows_texture", 33, 33)
    p = b.tracer()
    osc, P = b.oracle()
    assert_chain(p.ReadDenoiseGuides(specular_bounces=2), S.chain_guides(osc, P, 2), "before the move")
    # the mirror turns a little about the camera's up axis: other texels, and some pixels now look past the textured wall
    f, r, u = SC.camera_frame(33, 33)
    tris = b.tris.copy()
    n = -f + 0.2 * r
    n /= np.linalg.norm(n)
    tris["n"][:2] = n.astype(np.float32)
    tris["p"][:2] = SC.quad(3.0 * f, 50.0 * np.cross(u, n), 50.0 * u, n, SC.MIRROR)["p"]
    p.UpdateTriangles(0, tris["p"][:2].reshape(2, 9), tris["n"][:2].reshape(2, 9))
    from tests.test_refit_definition import lib_refit  # the host's refit of the same tree: what the oracle traverses
    r, nodes = lib_refit(b.bvh.nodes, b.bvh.tri_indices, tris)
    assert r == N.ADYPT_OK
    moved = O.Scene(nodes, b.bvh.tri_indices, tris, b.mats, textures=b.textures)
    g = S.chain_guides(moved, P, 2)
    assert not np.array_equal(g["albedo"], S.chain_guides(osc, P, 2)["albedo"])
    assert_chain(p.ReadDenoiseGuides(specular_bounces=2), g, "after the move")
    p.destroy()


def test_cli(scene_cache, tmp_path):
    import os
    import re
    import subprocess
    case = TINY0
    name, w, h, life, sub, spp = case
    inst, spec = G._instance(scene_cache, case)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    p.Trace(True, spp)
    den, g, info = p.Denoise(specular_bounces=4), p.ReadDenoiseGuides(specular_bounces=4), p.GetDenoiseSpecular()
    p.destroy()
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    out, d_exr, prefix = str(tmp_path / "o.exr"), str(tmp_path / "d.exr"), str(tmp_path / "g")
    r = subprocess.run([exe, spec.config_path, "--out", out, "--seed", str(SEED), "--spp", str(spp), "--denoise", d_exr, "--denoise-specular", "4", "--guides-out", prefix],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and "Saved denoised image (5 levels)" in text, text[-2000:]
    assert np.array_equal(bits(api.load_exr(d_exr)), bits(den)), "the denoised image"
    for k in ("albedo", "normal", "position"):
        assert np.array_equal(bits(api.load_exr("%s.%s.exr" % (prefix, k))), bits(g[k])), k
    assert np.array_equal(api.load_exr(prefix + ".chain.exr")[..., 0], g["chain"].astype(np.float32)), "chain classes"
    m = re.search(r"\[PT\]SPECULAR: bounces (\d+) followed (\d+) escaped (\d+) truncated (\d+) of (\d+) hit pixels, rays (\d+)\n", text)
    assert m, text[-2000:]
    got = [int(v) for v in m.groups()]
    assert got == [4, info["pixels_followed"], info["pixels_escaped"], info["pixels_truncated"], int(g["hit"].sum()), info["rays"]], (got, info)


def test_refusals(scene_cache):
    inst = make_instance(scene_cache, "tiny0", 96, 64)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    p.Trace(True, 2)
    ctx = p._ctx
    for bad in (0, 9, -1):
        sp = N.SpecularParams(bad)
        assert N.lib.adypt_denoise_specular(ctx, None, N.C.byref(sp)) == N.E_INVALID and b"bounces must be in [1, 8]" in N.lib.adypt_last_error(ctx)
        assert N.lib.adypt_read_denoise_guides_specular(ctx, bad, None, None, None, None) == N.E_INVALID
    assert N.lib.adypt_denoise_specular(ctx, None, None) == N.E_INVALID and b"specular is null" in N.lib.adypt_last_error(ctx)
    assert N.lib.adypt_get_denoise_specular(ctx, None) == N.E_INVALID
    assert p.GetDenoiseSpecular()["have"] == 0
    for kw in (dict(specular_bounces=9), dict(specular_bounces=-1), dict(specular_bounces=2, temporal=True), dict(specular_bounces=2, temporal=True, rectify=True)):
        with pytest.raises(ValueError):
            p.Denoise(**kw)
    with pytest.raises(ValueError):
        p.ReadDenoiseGuides(specular_bounces=9)
    bad_levels = N.DenoiseParams(0, 4.0, 0.1)
    sp = N.SpecularParams(2)
    assert N.lib.adypt_denoise_specular(ctx, N.C.byref(bad_levels), N.C.byref(sp)) == N.E_INVALID  # adypt_denoise's refusals, unchanged
    assert np.isfinite(p.Denoise(specular_bounces=2)).all()
    p.Trace(False)
    with pytest.raises(N.AdyptError) as e:
        p.Denoise(specular_bounces=2)
    assert e.value.code == N.E_STATE and "not path-traced" in str(e.value)
    p.destroy()
    # a shard context
    part = make_instance(scene_cache, "tiny0", 100, 75, rank=1, world=2)
    q = part.m_path_tracer
    q.SetNoiseStats(True)
    q.Trace(True, 3)
    with pytest.raises(N.AdyptError) as e:
        q.Denoise(specular_bounces=2)
    assert e.value.code == N.E_STATE and "tile shard" in str(e.value)
    q.destroy()
    # no camera
    b = SC.Built("mirror_under_sky", 32, 18)
    hs = api.HipScene()
    hs.Initialize(b.scene, b.bvh)
    t = api.HipPathTracer()
    t.Initialize(b.pt_params(), hs, 32, 18)
    with pytest.raises(N.AdyptError) as e:
        t.ReadDenoiseGuides(specular_bounces=2)
    assert e.value.code == N.E_STATE and "adypt_set_camera" in str(e.value)
    t.destroy()
