"""-m gpu: another set of triangles, of another length, and its tree, made on the device (include/adypt_hip.h adypt_set_triangles,
adypt_create_from_triangles; csrc/device/geometry.hip, the record: csrc/device/tri_record.hpp).  The device's records are held against those of a
context made by adypt_create (and those against numpy in tests/test_tri_record_definition.py), its node, index and Woop arrays against the host's
BuildLinear / BuildPLOC + woop_matrices byte for byte; rays and images against the CPU oracle on the host-built tree, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import refit_truth as T  # noqa: E402
from tests import tri_record_truth as R  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_gpu_rebuild import holds, host_linear  # noqa: E402
from tests.test_gpu_rebuild_ploc import host_ploc, levels_of  # noqa: E402
from tests.test_gpu_rebuild_split import holds_split, host_split  # noqa: E402
from tests.test_gpu_refit import PT, SPP, case_of, oracle_image, params, pose, same_woop, tracer, update  # noqa: E402
from tests.test_ploc_definition import DEGENERATE  # noqa: E402
from tests.test_refit_definition import lib_refit, same_bytes  # noqa: E402

_built = {}


def host_tree(tris, mats, method, radius=8, budget=0.0):
    """(WideBVH.BuildLinear or BuildPLOC of the triangles, their Woop data)"""
    b = api.WideBVH()
    s = api.Scene.FromArrays(tris, mats)
    if method == "linear":
        b.BuildLinear(s, api.InstanceConfig().bvh_params())
    else:
        b.BuildPLOC(s, api.InstanceConfig().bvh_params(), radius, budget)
    return b, api.woop_matrices(tris, b.tri_indices)


def no_bvh_tracer(case, scene, w=32, h=18, cls=api.HipPathTracer, **kw):
    """tracer() of tests/test_gpu_refit.py for a scene without a BVH"""
    hs = api.HipScene()
    hs.Initialize(scene)
    p = cls()
    p.Initialize(params(), hs, w, h, **kw)
    ip, iv = (case.ip, case.iv) if (w, h) == (32, 18) else api.camera_matrices(60.0, 30.0, -10.0, w, h)
    p.SetCamera(ip, iv, case.pos)
    return p


def info_of(b):
    return {"n_nodes": len(b.nodes) // 80, "n_refs": len(b.tri_indices), "levels": levels_of(b)}


def same_info(info, b):
    return all(info[k] == v for k, v in info_of(b).items()) and info["binary_depth"] >= info["levels"] - 1


# ---- 1. create from triangles equals the host ----
@pytest.mark.parametrize("name,method,budget", [(n, m, 0.0) for n in ("tiny2", "tiny0", "soup") for m in ("linear", "ploc")] + [("soup", "ploc", 0.3)])
def test_create_from_triangles_equals_the_host(name, method, budget, scene_cache):
    case = case_of(name, scene_cache)
    if budget:
        b, tris, woop, _ = host_split(case, name, "rest", budget)
    else:
        b, tris, woop = (host_linear if method == "linear" else host_ploc)(case, name, "rest")
    p = no_bvh_tracer(case, case.scene, method=method, radius=8, split_budget=budget)
    assert (holds_split if budget else holds)(p, b, woop), "nodes, indices, Woop data"
    assert same_info(p.build_info, b) and p.GetBVHSizes() == (len(b.nodes) // 80, len(b.tri_indices)) and p.GetTriangleCount() == len(tris)
    assert not budget or len(b.tri_indices) > len(tris)
    created = tracer(case, case.scene, case.bvh(48))
    assert created.build_info is None
    want = created.ReadTriangleRecords()
    created.destroy()
    got = p.ReadTriangleRecords()
    assert got.tobytes() == want.tobytes(), "the device's records equal adypt_create's"
    assert got.tobytes() == R.pack(case.tris, case.scene.materials, len(case.scene.textures))[0].tobytes()
    assert p.ReadTriangles().tobytes() == np.ascontiguousarray(case.tris).tobytes()
    p.destroy()


# ---- 2. one context through a chain of counts ----
def aimed_rays(tris, n, seed=5):
    """rays from one point outside the scene at points inside the triangles, ray i at triangle i % len(tris) (as test_degenerate_inputs aims them)"""
    rs = np.random.RandomState(seed)
    w = rs.dirichlet((2.0, 2.0, 2.0), size=n)
    p = tris["p"].astype(np.float64)[np.arange(n) % len(tris)]
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3], rays[:, 3] = (37.0, 41.0, 43.0), 1e-4
    rays[:, 4:7] = (p * w[:, :, None]).sum(axis=1) - np.array([37.0, 41.0, 43.0])
    return rays


# (count, soup seed, method, the least number of the 4096 rays on which the ORACLE hits, closest hit; any-hit rays hit on at least as many).
# The 5 000-triangle steps: rays_in_box alone, as the existing tests have it (> 1000).  Below: half rays_in_box, half aimed at the triangles.  The
# numbers are a little below what O.trace gives on the CPU for these inputs, closest hit and any hit alike — 5 000 / seed 7: 1227; 554: 2145; 1: 2214; 2: 2049;
# 257: 2097; 256: 2099; 255: 2090; 5 000 / seed 21: 1241
CHAIN = [(5000, 7, "ploc", 1200), (554, 8, "linear", 2100), (1, 3, "ploc", 2100), (2, 4, "ploc", 2040), (257, 9, "ploc", 2050), (256, 10, "linear", 2050), (255, 11, "ploc", 2050),
         (5000, 21, "ploc", 1200)]


def chain_rays(tris):
    if len(tris) >= 5000:
        return T.rays_in_box(tris, 4096)
    return np.concatenate([T.rays_in_box(tris, 2048), aimed_rays(tris, 2048)])


def test_one_context_through_a_chain_of_counts(scene_cache):
    case = case_of("soup", scene_cache)
    mats = case.scene.materials
    p = tracer(case, case.scene, case.bvh(48))
    for step, (n, seed, method, least) in enumerate(CHAIN):
        tris = T.soup(n, seed)
        tris["tc"] = np.random.RandomState(seed).uniform(0, 1, size=tris["tc"].shape).astype(np.float32)
        b, woop = host_tree(tris, mats, method)
        info = p.SetTriangles(tris, method=method)
        what = "step %d: %d triangles, %s" % (step, n, method)
        assert holds(p, b, woop), what
        assert same_info(info, b) and p.GetBVHSizes() == (len(b.nodes) // 80, n) and p.GetTriangleCount() == n, what
        assert p.ReadTriangles().tobytes() == tris.tobytes(), what
        assert p.ReadTriangleRecords().tobytes() == R.pack(tris, mats, 0)[0].tobytes(), what
        osc = O.Scene(b.nodes, b.tri_indices, tris, mats, woop=woop)
        rays = chain_rays(tris)
        for any_hit in (False, True):
            got, want = p.TraceRays(rays, with_stats=True, any_hit=any_hit), O.trace(osc, rays, stack_size=PT["stack_size"], any_hit=any_hit)
            print("%s any_hit %s: the oracle hits on %d of %d rays" % (what, any_hit, (want["tri_id"] >= 0).sum(), len(rays)))
            for f in api.HIT_DT.names:
                assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), "%s: %s (any_hit %s)" % (what, f, any_hit)
            assert (want["tri_id"] >= 0).sum() >= least, what
    p.destroy()


@pytest.mark.parametrize("what", sorted(DEGENERATE))
def test_degenerate_sets(what, scene_cache):
    case = case_of("soup", scene_cache)
    tris = DEGENERATE[what]()
    b, woop = host_tree(tris, case.scene.materials, "ploc")
    p = tracer(case, case.scene, case.bvh(48))
    info = p.SetTriangles(tris)
    assert holds(p, b, woop) and same_info(info, b) and p.GetTriangleCount() == len(tris)
    assert p.ReadTriangles().tobytes() == tris.tobytes()
    rays = aimed_rays(tris, 4096)
    got, want = p.TraceRays(rays, with_stats=True), O.trace(O.Scene(b.nodes, b.tri_indices, tris, case.scene.materials, woop=woop), rays, stack_size=PT["stack_size"])
    for f in api.HIT_DT.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    assert (want["tri_id"] >= 0).sum() >= 4000  # (on the CPU the oracle hits on all 4096 aimed rays of every one of these sets)
    p.destroy()


# ---- 3. images ----
def thinned_wave(case):
    """the wave pose with every third triangle dropped"""
    t = pose(case.tris)
    return np.ascontiguousarray(t[np.arange(len(t)) % 3 != 2])


def thinned_image(case, name, sobol_matrices):
    if name not in _built:
        tris = thinned_wave(case)
        b, woop = host_tree(tris, case.scene.materials, "ploc")
        image = oracle_image(case, b.nodes, b.tri_indices, tris, sobol_matrices)
        image.setflags(write=False)
        _built[name] = (tris, b, woop, image)
    return _built[name]


@pytest.mark.parametrize("variant", ["fused", "launch_per_bounce", "fused_remap", "launch_per_bounce_shade_bin"])
@pytest.mark.parametrize("name", ["soup", "tiny0"])
def test_image_after_set_triangles(name, variant, scene_cache, sobol_matrices, monkeypatch):
    case = case_of(name, scene_cache)
    if variant.endswith("remap"):
        monkeypatch.setenv("ADYPT_REF_TRIANGLES_MAX_MB", "0")  # no per-reference records: k_path remaps through the new index array
    if variant.endswith("shade_bin"):
        monkeypatch.setenv("ADYPT_SHADE_BIN", "1")  # the context keeps a class byte per triangle, which k_shade sorts by: k_pack_triangles writes those too
    tris, b, woop, want = thinned_image(case, name, sobol_matrices)
    p = tracer(case, case.scene, case.bvh(48))
    fused = variant.startswith("fused")
    if not fused:
        p.SetFusedBounces(False)
    p.Trace(True, 2)  # (the old scene has been rendered: per-reference records, primary-hit cache and image are its)
    p.SetTriangles(tris)
    assert p.GetSPP() == 0 and p.GetTriangleCount() == len(tris) < len(case.tris)
    p.Trace(True, SPP)
    assert p.GetFusedBounces() == fused
    assert np.array_equal(bits(p.ReadResult()), bits(want)), "the image of the new triangles"
    assert not np.array_equal(bits(want), bits(oracle_image(case, case.bvh(48).nodes, case.bvh(48).tri_indices, case.tris, sobol_matrices)))  # the change shows
    p.destroy()


# ---- 4. afterwards the geometry calls work on the new count ----
def test_geometry_calls_after_set_triangles(scene_cache):
    case = case_of("soup", scene_cache)
    tris = T.soup(554, 8)
    mats = case.scene.materials
    b, woop = host_tree(tris, mats, "ploc")
    p = tracer(case, case.scene, case.bvh(48))
    p.SetTriangles(tris)
    # a range of the old count is none of the new
    with pytest.raises(N.AdyptError) as e:
        update(p, case.tris, first=0, count=5000)
    assert e.value.code == N.E_INVALID and "554" in str(e.value)
    with pytest.raises(N.AdyptError):
        update(p, case.tris, first=600, count=10)
    assert holds(p, b, woop)
    # the refit of the new tree is the host's
    moved = T.jitter(tris)
    update(p, moved)
    r, want = lib_refit(b.nodes, b.tri_indices, moved)
    assert r == N.ADYPT_OK
    nodes, got_woop = p.ReadBVH()
    assert same_bytes(nodes, want) and same_woop(got_woop, api.woop_matrices(moved, b.tri_indices))
    assert p.ReadTriangles().tobytes() == moved.tobytes()
    # the cost of the refitted tree, a rebuild, and the policy that always rebuilds
    refitted = api.WideBVH()
    refitted.nodes, refitted.tri_indices = want, b.tri_indices
    cost = p.GetTreeCost()
    assert (cost["inner_q"], cost["leaf_q"], cost["n_nodes"]) == tuple(refitted.Cost()[k] for k in ("inner_q", "leaf_q", "n_nodes"))
    lb, lwoop = host_tree(moved, mats, "linear")
    info = p.RebuildBVH()
    assert holds(p, lb, lwoop) and same_info(info, lb)
    again = T.wave(tris)
    out = p.UpdateTriangles(0, again["p"].reshape(-1, 9), rebuild_above=0.0, method="ploc")
    pb, pwoop = host_tree(again, mats, "ploc")
    assert out["rebuilt"] == 1 and holds(p, pb, pwoop) and same_info(out["rebuild"], pb)
    assert (out["now"]["inner_q"], out["now"]["leaf_q"]) == tuple(pb.Cost()[k] for k in ("inner_q", "leaf_q"))
    assert p.GetTriangleCount() == 554
    p.destroy()


# ---- 5. state ----
@pytest.mark.parametrize("setting", ["frozen_blocks", "lookahead"])
def test_set_triangles_in_the_middle_of_an_accumulation(setting, scene_cache, sobol_matrices):
    case = case_of("tiny0", scene_cache)
    tris, b, woop, want = thinned_image(case, "tiny0", sobol_matrices)
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
    stats = p.GetNoiseStats()
    p.SetTriangles(tris)
    assert p.GetSPP() == 0 and p.GetLookaheadFrames() == 0 and p.GetNoiseStats() == stats
    if setting == "lookahead":
        for _ in range(SPP):
            p.Trace(True, 1)
    else:
        p.Trace(True, SPP)
    assert p.GetSPP() == SPP
    if setting == "frozen_blocks":
        assert (p.ReadBlockSPP()[1] == SPP).all()  # thawed
    assert np.array_equal(bits(p.ReadResult()), bits(want))
    p.destroy()


# ---- 6. refusals change nothing ----
def test_refusals_change_nothing(scene_cache, sobol_matrices):
    case = case_of("tiny0", scene_cache)
    b = case.bvh(48)
    p = tracer(case, case.scene, b)
    p.Trace(True, SPP)
    before = p.ReadResult()
    sizes, woop = p.GetBVHSizes(), api.woop_matrices(case.tris, b.tri_indices)
    good = T.soup(300, 12)
    nan = good.copy()
    nan["p"][123, 1] = np.nan  # one vertex
    cases = [("a null pointer", lambda: p.SetTriangles(None)),
             ("no triangles", lambda: p.SetTriangles(good[:0])),
             ("method 2", lambda: p._call("set_triangles", good.ctypes.data, len(good), None, 2, 8, 0.0, None)),
             ("radius 0", lambda: p.SetTriangles(good, radius=0)),
             ("radius 33", lambda: p.SetTriangles(good, radius=33)),
             ("budget 1.5", lambda: p.SetTriangles(good, split_budget=1.5)),
             ("a budget with method 0", lambda: p.SetTriangles(good, method="linear", split_budget=0.25)),
             ("a NaN vertex", lambda: p.SetTriangles(nan)),
             ("a NaN vertex, linear", lambda: p.SetTriangles(nan, method="linear"))]
    for what, call in cases:
        with pytest.raises(N.AdyptError) as e:
            call()
        assert e.value.code == N.E_INVALID, what
        assert p.GetTriangleCount() == len(case.tris) and p.GetBVHSizes() == sizes, what
    assert holds(p, b, woop) and p.ReadTriangles().tobytes() == np.ascontiguousarray(case.tris).tobytes()
    assert p.GetSPP() == SPP and np.array_equal(bits(p.ReadResult()), bits(before)), "the image is still there"
    p.Reset()
    p.Trace(True, SPP)
    assert np.array_equal(bits(p.ReadResult()), bits(before)), "the context renders what it rendered before"
    p.destroy()
    # adypt_create_from_triangles: no context
    for what, scene, kw in (("a NaN vertex", case.moved_scene(nan), {}), ("radius 33", case.scene, dict(radius=33)), ("budget 1.5", case.scene, dict(split_budget=1.5)),
                            ("a budget with method 0", case.scene, dict(method="linear", split_budget=0.25)), ("radius 0", case.scene, dict(radius=0))):
        hs = api.HipScene()
        hs.Initialize(scene)
        q = api.HipPathTracer()
        with pytest.raises(N.AdyptError) as e:
            q.Initialize(params(), hs, 32, 18, **kw)
        assert e.value.code == N.E_INVALID and not q._h, what


# ---- 7. multi ----
def test_two_shards_on_one_device(scene_cache, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = case_of("soup", scene_cache)
    tris = thinned_wave(case)
    b, woop = host_tree(tris, case.scene.materials, "ploc")
    w, h = 64, 36  # 2 x 2 blocks: both shards own some
    single = tracer(case, case.scene, case.bvh(48), w, h)
    multi = tracer(case, case.scene, case.bvh(48), w, h, cls=api.MultiPathTracer, devices=(0, 0))
    from_triangles = no_bvh_tracer(case, case.moved_scene(tris), w, h, cls=api.MultiPathTracer, devices=(0, 0))
    assert multi.DeviceCount() == from_triangles.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in multi._contexts())
    assert same_info(from_triangles.build_info, b)
    for t in (single, multi):
        t.Trace(True, 2)
        info = t.SetTriangles(tris)
        assert t.GetSPP() == 0 and same_info(info, b)
    images = []
    for t in (single, multi, from_triangles):
        for c in t._contexts():
            nodes, got_woop = np.zeros(len(b.nodes), np.uint8), np.zeros((len(tris), 12), np.float32)
            assert N.lib.adypt_get_triangle_count(c) == len(tris)
            N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, got_woop.ctypes.data), c)
            assert same_bytes(nodes, b.nodes) and same_woop(got_woop, woop)
        t.Trace(True, SPP)
        images.append(t.ReadResult())
        t.destroy()
    assert np.array_equal(bits(images[0]), bits(images[1])), "two shards equal the single context"
    assert np.array_equal(bits(images[0]), bits(images[2])), "created from the triangles"
