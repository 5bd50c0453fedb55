"""-m gpu: a new tree built on the device (include/adypt_hip.h adypt_rebuild_bvh ...; csrc/device/build.hip).  The device's node, index and Woop arrays are
held against the host's adypt_bvh_build_linear + adypt_woop_matrices byte for byte (and that against numpy and the SBVH tree in
tests/test_lbvh_definition.py); rays and images after a rebuild against the CPU oracle on the host-built linear tree, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import refit_truth as T  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_gpu_refit import PT, SPP, case_of, oracle_image, pose, same_woop, tracer, update  # noqa: E402
from tests.test_lbvh_definition import shared_centroid  # noqa: E402
from tests.test_refit_definition import lib_refit, same_bytes  # noqa: E402

_linear, _images = {}, {}


def host_linear(case, name, which):
    """(WideBVH.BuildLinear of the pose, its triangles, their Woop data); shared and never written"""
    if (name, which) not in _linear:
        tris = case.tris if which == "rest" else pose(case.tris)
        b = api.WideBVH()
        b.BuildLinear(api.Scene.FromArrays(tris, case.scene.materials), api.InstanceConfig().bvh_params())
        b.nodes.setflags(write=False)
        _linear[name, which] = (b, tris, api.woop_matrices(tris, b.tri_indices))
    return _linear[name, which]


def holds(p, b, woop):
    nodes, got_woop = p.ReadBVH()
    return same_bytes(nodes, b.nodes) and np.array_equal(p.ReadTriIndices(), b.tri_indices) and same_woop(got_woop, woop)


@pytest.mark.parametrize("name", ["tiny2", "tiny0", "soup"])
def test_device_equals_host(name, scene_cache):
    case = case_of(name, scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    info = p.RebuildBVH()
    b, tris, woop = host_linear(case, name, "rest")
    assert p.GetBVHSizes() == (len(b.nodes) // 80, len(tris)) == (info["n_nodes"], info["n_refs"])
    assert holds(p, b, woop), "the rest pose"
    assert info["levels"] == int(T.depths(np.ascontiguousarray(b.nodes).view(O.NODE_DT)).max()) + 1 and info["binary_depth"] >= info["levels"] - 1
    ms = p.GetRebuildTiming()
    assert ms["total"] > 0.0 and all(ms[k] >= 0.0 for k in ms)
    update(p, pose(case.tris))
    p.RebuildBVH()
    b, _, woop = host_linear(case, name, "wave")
    assert holds(p, b, woop), "after the wave pose"
    p.destroy()


@pytest.mark.parametrize("name", ["tiny2", "tiny0", "soup"])
def test_rays_after_a_rebuild(name, scene_cache):
    case = case_of(name, scene_cache)
    b, tris, woop = host_linear(case, name, "wave")
    osc = O.Scene(b.nodes, b.tri_indices, tris, case.scene.materials, woop=woop)
    rays = T.rays_in_box(tris, 4096)
    p = tracer(case, case.scene, case.bvh(48))
    update(p, tris)
    p.RebuildBVH()
    for any_hit in (False, True):
        got, want = p.TraceRays(rays, with_stats=True, any_hit=any_hit), O.trace(osc, rays, stack_size=PT["stack_size"], any_hit=any_hit)
        for f in api.HIT_DT.names:
            assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), "%s (any_hit %s)" % (f, any_hit)
        assert name == "tiny2" or (want["tri_id"] >= 0).sum() > 1000
    p.destroy()


def linear_image(case, name, sobol_matrices):
    if name not in _images:
        b, tris, _ = host_linear(case, name, "wave")
        _images[name] = oracle_image(case, b.nodes, b.tri_indices, tris, sobol_matrices)
        _images[name].setflags(write=False)
    return _images[name]


@pytest.mark.parametrize("variant", ["fused", "launch_per_bounce", "fused_remap", "launch_per_bounce_remap"])
@pytest.mark.parametrize("name", ["tiny0", "soup"])
def test_image_after_a_rebuild(name, variant, scene_cache, sobol_matrices, monkeypatch):
    case = case_of(name, scene_cache)
    if variant.endswith("remap"):
        monkeypatch.setenv("ADYPT_REF_TRIANGLES_MAX_MB", "0")  # no per-reference records: k_path remaps through the new index array
    p = tracer(case, case.scene, case.bvh(48))
    fused = variant.startswith("fused")
    if not fused:
        p.SetFusedBounces(False)
    p.Trace(True, 2)  # (the old tree has been rendered: per-reference records, primary-hit cache and image are its)
    update(p, pose(case.tris))
    p.RebuildBVH()
    assert p.GetSPP() == 0
    p.Trace(True, SPP)
    assert p.GetFusedBounces() == fused
    assert np.array_equal(bits(p.ReadResult()), bits(linear_image(case, name, sobol_matrices))), "the image on the rebuilt tree"
    p.destroy()


def fresh_image(case, name):
    """the image a context created with the host-built linear tree of the wave pose renders"""
    b, tris, _ = host_linear(case, name, "wave")
    p = tracer(case, case.moved_scene(tris), b)
    p.Trace(True, SPP)
    image = p.ReadResult()
    p.destroy()
    return image


@pytest.mark.parametrize("setting", ["frozen_blocks", "lookahead"])
def test_rebuild_in_the_middle_of_an_accumulation(setting, scene_cache):
    case = case_of("tiny0", scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    if setting == "frozen_blocks":
        p.SetNoiseStats(True)
        r = p.TraceAdaptive(1e30, min_spp=2, max_spp=8, check_every=2)
        assert r["blocks_frozen"] == r["blocks"] > 0 and (p.ReadBlockSPP()[1] == 2).all()
    else:
        p.SetFramesInFlight(4)
        p.SetLookahead(True)
        p.Trace(True, 1)
        assert p.GetLookaheadFrames() == 3
    update(p, pose(case.tris))
    if setting == "lookahead":  # frames parked ahead again, now of the refitted tree: the rebuild must drop them too
        p.Trace(True, 1)
        assert p.GetLookaheadFrames() == 3
    p.RebuildBVH()
    assert p.GetSPP() == 0 and p.GetLookaheadFrames() == 0
    if setting == "lookahead":
        for _ in range(SPP):
            p.Trace(True, 1)
    else:
        p.Trace(True, SPP)
    assert p.GetSPP() == SPP
    if setting == "frozen_blocks":
        assert (p.ReadBlockSPP()[1] == SPP).all()  # thawed
    assert np.array_equal(bits(p.ReadResult()), bits(fresh_image(case, "tiny0"))), setting
    p.destroy()


@pytest.mark.parametrize("name", ["tiny0", "soup"])
def test_refit_after_a_rebuild(name, scene_cache):
    case = case_of(name, scene_cache)
    b, _, _ = host_linear(case, name, "rest")
    p = tracer(case, case.scene, case.bvh(48))
    p.RebuildBVH()
    moved = T.jitter(case.tris)
    update(p, moved)
    r, want = lib_refit(b.nodes, b.tri_indices, moved)
    assert r == N.ADYPT_OK
    nodes, woop = p.ReadBVH()
    assert same_bytes(nodes, want) and same_woop(woop, api.woop_matrices(moved, b.tri_indices)) and np.array_equal(p.ReadTriIndices(), b.tri_indices)
    p.destroy()


def test_sizes_change(scene_cache):
    case = case_of("tiny0", scene_cache)
    split = case.bvh(48)
    assert len(split.tri_indices) > len(case.tris)  # spatial splits
    p = tracer(case, case.scene, split)
    assert p.GetBVHSizes() == (len(split.nodes) // 80, len(split.tri_indices))
    nodes, woop = p.ReadBVH()  # (a context that was never rebuilt: what was uploaded)
    assert same_bytes(nodes, split.nodes) and np.array_equal(p.ReadTriIndices(), split.tri_indices) and len(woop) == len(split.tri_indices)
    info = p.RebuildBVH()
    assert info["n_refs"] == len(case.tris) and p.GetBVHSizes() == (info["n_nodes"], len(case.tris))
    assert len(p.ReadBVH()[1]) == len(case.tris) == len(p.ReadTriIndices())
    p.destroy()


class Loose:
    """what tracer() asks of a case, for triangles that come from no scene file"""

    def __init__(self, tris):
        self.tris = tris
        self.scene = api.Scene.FromArrays(tris, T.soup_material())
        self.ip, self.iv = api.camera_matrices(60.0, 30.0, -10.0, 32, 18)
        self.pos = np.zeros(3, np.float32)


@pytest.mark.parametrize("what", ["one", "shared_centroid"])
def test_degenerate_inputs(what):
    tris = T.soup(1, 3) if what == "one" else shared_centroid(300, 6)
    case = Loose(tris)
    sbvh = api.WideBVH()
    cfg = api.InstanceConfig().bvh_params()
    sbvh.Build(case.scene, cfg)
    b = api.WideBVH()
    b.BuildLinear(case.scene, cfg)
    p = tracer(case, case.scene, sbvh)
    info = p.RebuildBVH()
    assert holds(p, b, api.woop_matrices(tris, b.tri_indices))
    assert what != "one" or (info["n_nodes"], info["levels"], info["binary_depth"]) == (1, 1, 0)
    rays = np.zeros((len(tris) + 7, 8), np.float32)
    rays[:, :3], rays[:, 3] = (37.0, 41.0, 43.0), 1e-4
    rays[:len(tris), 4:7] = (tris["p"][:, 0].astype(np.float64) * 0.25 + tris["p"].astype(np.float64).mean(axis=1) * 0.75) - np.array([37.0, 41.0, 43.0])
    rays[len(tris):, 4:7] = (1.0, 0.5, 0.25)  # away from everything
    got, want = p.TraceRays(rays, with_stats=True), O.trace(O.Scene(b.nodes, b.tri_indices, tris, case.scene.materials), rays, stack_size=PT["stack_size"])
    for f in api.HIT_DT.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    assert (want["tri_id"][:len(tris)] >= 0).sum() >= max(1, len(tris) // 2) and (want["tri_id"][len(tris):] < 0).all()
    p.destroy()


def test_refusals_change_nothing(scene_cache):
    case = case_of("tiny0", scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    p.Trace(True, SPP)
    image, before, idx = p.ReadResult(), p.ReadBVH(), p.ReadTriIndices()
    for tri_sah, node_sah in ((0.0, 1.0), (0.3, -1.0), (float("nan"), 1.0), (0.3, float("inf"))):
        cfg = api.InstanceConfig().bvh_params()
        cfg.triangle_sah, cfg.node_sah = tri_sah, node_sah
        with pytest.raises(N.AdyptError) as e:
            p.RebuildBVH(cfg)
        assert e.value.code == N.E_INVALID
    with pytest.raises(N.AdyptError) as e:
        p.GetRebuildTiming()  # nothing has been rebuilt
    assert e.value.code == N.E_STATE
    now = p.ReadBVH()
    assert p.GetSPP() == SPP and np.array_equal(bits(p.ReadResult()), bits(image))
    assert same_bytes(now[0], before[0]) and np.array_equal(bits(now[1]), bits(before[1])) and np.array_equal(p.ReadTriIndices(), idx)
    p.Reset()
    p.Trace(True, SPP)
    assert np.array_equal(bits(p.ReadResult()), bits(image))  # the old tree is in place and usable
    # other costs are another tree, and the host's for them
    cfg = api.InstanceConfig().bvh_params()
    cfg.triangle_sah, cfg.node_sah, cfg.max_spatial_depth = 1.0, 0.25, 7  # (the depth is ignored)
    p.RebuildBVH(cfg)
    b = api.WideBVH()
    b.BuildLinear(api.Scene.FromArrays(case.tris, case.scene.materials), cfg)
    assert holds(p, b, api.woop_matrices(case.tris, b.tri_indices))
    assert not same_bytes(b.nodes, host_linear(case, "tiny0", "rest")[0].nodes)
    p.destroy()


def test_two_shards_on_one_device(scene_cache, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = case_of("soup", scene_cache)
    b, tris, woop = host_linear(case, "soup", "wave")
    w, h = 64, 36  # 2 x 2 blocks: both shards own some
    single = tracer(case, case.scene, case.bvh(48), w, h)
    multi = tracer(case, case.scene, case.bvh(48), w, h, cls=api.MultiPathTracer, devices=(0, 0))
    assert multi.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in multi._contexts())
    for t in (single, multi):
        t.Trace(True, 2)
        update(t, tris)
        info = t.RebuildBVH()
        assert t.GetSPP() == 0 and info["n_refs"] == len(tris)
        t.Trace(True, SPP)
    assert holds(single, b, woop)
    a = single.ReadBVH()
    for c in multi._contexts():  # every device rebuilt its own copy
        nodes, got_woop, idx = np.zeros_like(a[0]), np.zeros_like(a[1]), np.zeros(len(tris), np.int32)
        N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, got_woop.ctypes.data), c)
        N.check(N.lib.adypt_read_tri_indices(c, idx.ctypes.data), c)
        assert same_bytes(nodes, a[0]) and np.array_equal(bits(got_woop), bits(a[1])) and np.array_equal(idx, b.tri_indices)
    assert np.array_equal(bits(multi.ReadResult()), bits(single.ReadResult()))
    assert not np.array_equal(bits(single.ReadResult()), np.zeros_like(bits(single.ReadResult())))
    multi.destroy()
    single.destroy()
