"""-m gpu: the geometry kernels past their workgroup, stride and sort thresholds (csrc/device/build.hip, refit.hip, pose.hip, geometry.hip, the motion
snapshot of denoise.hip).  The scenes are tests/geometry_scale_scenes.py's — 65 538, 262 146 and 1 048 578 triangles with two outliers that only the
second round of a reduction's loop reaches (what makes them sharp is held on the CPU in tests/test_geometry_scale_inputs.py).  Everything is held byte
for byte against the host's deterministic counterpart, each of which is held against numpy at small sizes elsewhere in the suite: BuildLinear / BuildPLOC +
woop_matrices, adypt_bvh_refit, tri_record_truth.pack, adypt_pose_triangles, WideBVH.Cost, the CPU oracle's rays and primary frame, and
temporal_motion_truth.previous_point.  Every host truth is built once per (count, method) and never written.  One test per (operation, count): a
failure, or a fault, names the narrowest thing.
Which test would fail if a branch were wrong:
    the second pass of the box reduction going round its loop twice (n > 65 536): test_rebuild_equals_the_host[65538-*] (the outliers lie in partial box 256:
        other keys, another tree), -split for the scene box of the pre-split (another level, other references)
    the first pass capped at 1 024 workgroups (n > 262 144): test_rebuild_equals_the_host[262146-*] (the outliers are the second round of threads 0 and 1
        of workgroup 0), -split for k_ref_centroid_box and k_centroid_box<kOfTriangles>
    rocPRIM's Onesweep (n > merge_sort_limit): test_rebuild_equals_the_host[1048578-*] (the reference order is the sorted keys' low words)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import geometry_scale_scenes as S  # noqa: E402
from tests import pose_truth as P  # noqa: E402
from tests import refit_truth as T  # noqa: E402
from tests import temporal_motion_truth as TM  # noqa: E402
from tests import tri_record_truth as R  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_gpu_pose import gentle, host_posed, with_zero  # noqa: E402
from tests.test_gpu_rebuild import Loose, holds  # noqa: E402
from tests.test_gpu_rebuild_split import holds_split  # noqa: E402
from tests.test_gpu_refit import PT, case_of, params, same_woop, tracer, update  # noqa: E402
from tests.test_gpu_set_triangles import no_bvh_tracer, same_info  # noqa: E402
from tests.test_presplit_definition import lib_refs  # noqa: E402
from tests.test_refit_definition import lib_refit, same_bytes  # noqa: E402

SMALL, MIDDLE, TOP = S.COUNTS
METHODS = ("linear", "ploc", "split")
BUILD = {"linear": dict(method="linear"), "ploc": dict(method="ploc", radius=8), "split": dict(method="ploc", radius=8, split_budget=S.SPLIT_BUDGET)}
N_MATRICES = 300
_cases, _levels, _refits, _records, _posed = {}, {}, {}, {}, {}


# ---- the truths: once per key, shared, never written ----
def case(n):
    """what tracer() and no_bvh_tracer() ask of a case, for far_ends(n)"""
    if n not in _cases:
        _cases[n] = Loose(S.far_ends(n))
    return _cases[n]


def presplit_of(n):
    """(the level the host chooses for SPLIT_BUDGET, the triangles it splits)"""
    if n not in _levels:
        level, ref_tri, _ = lib_refs(S.far_ends(n), S.SPLIT_BUDGET)
        _levels[n] = (level, int((np.bincount(ref_tri, minlength=n) > 1).sum()))
    return _levels[n]


def moved(n, which):
    if (n, which) not in _posed:
        t = T.wave(S.far_ends(n))
        if which == "further":  # the wave of the wave, for a range of its own
            t = T.wave(t)
        t.setflags(write=False)
        _posed[n, which] = t
    return _posed[n, which]


def refit_of(n, method, tris, key):
    """(adypt_bvh_refit of the host's tree for the triangles, their Woop data in its order)"""
    if (n, method, key) not in _refits:
        b, _ = S.host_tree(n, method)
        r, nodes = lib_refit(b.nodes, b.tri_indices, tris)
        assert r == N.ADYPT_OK
        nodes.setflags(write=False)
        _refits[n, method, key] = (nodes, api.woop_matrices(tris, b.tri_indices))
    return _refits[n, method, key]


def records_of(n, tris, key):
    if (n, key) not in _records:
        rec = R.pack(tris, T.soup_material(), 0)[0]
        rec.setflags(write=False)
        _records[n, key] = rec
    return _records[n, key]


def uploaded(n, w=32, h=18):
    """a context made by adypt_create with the host's linear tree: nothing of the device's build runs"""
    c = case(n)
    return tracer(c, c.scene, S.host_tree(n, "linear")[0], w, h)


def expect(p, b, woop, method, what):
    assert (holds_split if method == "split" else holds)(p, b, woop), what + ": nodes, reference order, Woop data" + (", reference boxes" if method == "split" else "")
    assert p.GetBVHSizes() == (len(b.nodes) // 80, len(b.tri_indices)), what
    if method != "split":
        assert p.ReadRefBoxes() is None, what


def expect_refit(p, n, method, tris, key, what):
    b, _ = S.host_tree(n, method)
    want_nodes, want_woop = refit_of(n, method, tris, key)
    nodes, woop = p.ReadBVH()
    assert same_bytes(nodes, want_nodes), what + ": nodes"
    assert same_woop(woop, want_woop), what + ": Woop data"
    assert np.array_equal(p.ReadTriIndices(), b.tri_indices), what + ": the reference order stays"


def host_cost(nodes):
    b = api.WideBVH()
    b.nodes = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    return b.Cost()


# ---- a. a rebuild equals the host ----
# The first tree of a count comes three ways, one per method: "linear" — creation from the triangles; "ploc" — SetTriangles on a context that held the
# 5 000-triangle soup, whose scratch (keys, sort_tmp, the PLOC lists) has to grow across the thresholds; "split" — RebuildBVH on a context that was
# given the host's linear tree.  Then RebuildBVH twice more: k_emit's queue order is arrival order, its output must not be.
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", S.COUNTS)
def test_rebuild_equals_the_host(n, method, scene_cache):
    c, tris = case(n), S.far_ends(n)
    b, woop = S.host_tree(n, method)
    presplit = presplit_of(n) if method == "split" else (-1, 0)
    if method == "split":
        assert len(b.tri_indices) > n and np.array_equal(b.ref_boxes.shape, (len(b.tri_indices), 6))
    if method == "linear":
        p = no_bvh_tracer(c, c.scene, **BUILD[method])
        info = p.build_info
    elif method == "ploc":
        soup = case_of("soup", scene_cache)
        p = tracer(soup, soup.scene, soup.bvh(48))
        p.RebuildBVH(**BUILD[method])  # (the scratch of 5 000 triangles is there)
        info = p.SetTriangles(tris, **BUILD[method])
    else:
        p = uploaded(n)
        info = p.RebuildBVH(**BUILD[method])
    print("%d %s: %s, presplit %s" % (n, method, info, presplit))
    expect(p, b, woop, method, "the first tree")
    assert same_info(info, b) and p.GetTriangleCount() == n
    assert p.GetRebuildPresplit() == presplit
    if method != "split":  # (the records: what the build read)
        assert p.ReadTriangleRecords().tobytes() == records_of(n, tris, "rest").tobytes()
    for k in range(2):
        again = p.RebuildBVH(**BUILD[method])
        expect(p, b, woop, method, "RebuildBVH %d" % k)
        assert again == info and p.GetRebuildPresplit() == presplit
    p.destroy()


# ---- b. rays after it ----
# Of the 4 096 rays the ORACLE hits, on the CPU, closest hit and any hit alike, on 1 718 at 65 538, on 1 886 at 262 146 and on 1 963 at 1 048 578 (either tree): at
# least 1 500 are asked for.  The context is created from the triangles: the tree the rays cross is the device's own.
RAYS = [(SMALL, "linear"), (MIDDLE, "ploc"), (TOP, "linear"), (TOP, "split")]


@pytest.mark.parametrize("n,method", RAYS)
def test_rays_after_a_rebuild(n, method):
    c, tris = case(n), S.far_ends(n)
    b, woop = S.host_tree(n, method)
    osc = O.Scene(b.nodes, b.tri_indices, tris, c.scene.materials, woop=woop)
    rays = T.rays_in_box(tris, 4096)
    p = no_bvh_tracer(c, c.scene, **BUILD[method])
    for any_hit in (False, True):
        got, want = p.TraceRays(rays, with_stats=True, any_hit=any_hit), O.trace(osc, rays, stack_size=PT["stack_size"], any_hit=any_hit)
        print("%d %s any_hit %s: the oracle hits on %d of %d rays" % (n, method, any_hit, (want["tri_id"] >= 0).sum(), len(rays)))
        for f in api.HIT_DT.names:
            assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), "%s (any_hit %s)" % (f, any_hit)
        assert (want["tri_id"] >= 0).sum() >= 1500
    p.destroy()


# ---- c. refit at scale ----
FIRST, COUNT = 262100, 300


@pytest.mark.parametrize("method", ["linear", "split"])
def test_refit_at_scale(method):
    n = TOP
    tris, wave, further = S.far_ends(n), moved(n, "wave"), moved(n, "further")
    p = uploaded(n)
    if method == "split":
        p.RebuildBVH(**BUILD[method])
        assert p.ReadRefBoxes() is not None
        # the rest pose again: the tree stays, its leaves bound whole triangles from here on (as tests/test_gpu_rebuild_split.py has it at 5 000)
        update(p, tris)
        expect_refit(p, n, method, tris, "rest", "the rest pose on the split tree")
        assert p.ReadRefBoxes() is None
        assert not same_bytes(refit_of(n, method, tris, "rest")[0], S.host_tree(n, method)[0].nodes)
    update(p, wave)
    expect_refit(p, n, method, wave, "wave", "all triangles")
    assert p.ReadTriangleRecords().tobytes() == records_of(n, wave, "wave").tobytes(), "the records of all triangles"
    ms = p.GetRefitTiming()
    assert ms["total"] > 0.0 and ms["nodes"] > 0.0
    # a range in the middle, moved further
    partly = np.array(wave)
    partly[FIRST:FIRST + COUNT] = further[FIRST:FIRST + COUNT]
    update(p, partly, first=FIRST, count=COUNT)
    expect_refit(p, n, method, partly, "partly", "a range of %d from %d" % (COUNT, FIRST))
    assert p.ReadTriangleRecords().tobytes() == R.pack(partly, T.soup_material(), 0)[0].tobytes(), "the records after the range"
    assert not same_bytes(refit_of(n, method, partly, "partly")[0], refit_of(n, method, wave, "wave")[0])
    p.destroy()


# ---- d. pose at scale ----
def binding_of(kind, n):
    if kind == "parts":
        return {"parts": P.parts_of(n, N_MATRICES)}
    j, w = P.skin_of(n, N_MATRICES)
    return {"joints": j, "weights": w}


@pytest.mark.parametrize("kind", ["parts", "skin"])
def test_pose_at_scale(kind):
    n = TOP
    tris = S.far_ends(n)
    binding = binding_of(kind, n)
    p = uploaded(n)
    rest = p.ReadTriangleRecords()
    assert rest.tobytes() == records_of(n, tris, "rest").tobytes()
    if kind == "parts":
        p.BindParts(binding["parts"], N_MATRICES)
    else:
        p.BindSkin(binding["joints"], binding["weights"], N_MATRICES)
    got = p.GetPoseBinding()
    assert (got["kind"], got["n_matrices"], got["n_tris"]) == (1 if kind == "parts" else 2, N_MATRICES, n)
    # the set with the zero matrix, then the gentle one: the second pose starts from the rest pose again, not from the first
    for name, mats in (("with_zero", with_zero(N_MATRICES)), ("gentle", gentle(N_MATRICES))):
        assert p.Pose(mats) is None
        posed = host_posed(tris, mats, **binding)
        rec = p.ReadTriangleRecords()
        assert rec.tobytes() == R.pack(posed, T.soup_material(), 0)[0].tobytes(), "%s, %s: the records" % (kind, name)
        assert np.array_equal(rec[:, 18:], rest[:, 18:]), "%s, %s: words 18 .." % (kind, name)
        assert not np.array_equal(rec[:, :18], rest[:, :18])
    expect_refit(p, n, "linear", posed, kind, kind + ", the gentle matrices")
    p.Pose(gentle(N_MATRICES))
    assert p.ReadTriangleRecords().tobytes() == rec.tobytes(), "the same pose twice"
    p.destroy()


# ---- e. the tree's cost at scale ----
@pytest.mark.parametrize("n", [MIDDLE, TOP])
def test_tree_cost_at_scale(n):
    c = case(n)
    b, _ = S.host_tree(n, "linear")
    p = no_bvh_tracer(c, c.scene, **BUILD["linear"])
    got, want = p.GetTreeCost(), b.Cost()
    print(n, "after the rebuild:", got)
    assert got == want and got["n_nodes"] == len(b.nodes) // 80 and got["inner_q"] > 0 and got["leaf_q"] > 0
    assert p.GetTreeCost() == want  # (the sums start from zero every time)
    wave = moved(n, "wave")
    update(p, wave)
    got, want = p.GetTreeCost(), host_cost(refit_of(n, "linear", wave, "wave")[0])
    print(n, "after the update:", got)
    assert got == want and got != b.Cost()
    p.destroy()


# ---- f. the motion snapshot at scale ----
W, H = 64, 36
CAMERA = (0.0, 0.0, 30.0)


def test_motion_snapshot_at_scale():
    """64 x 36, no sub-pixel jitter, the camera at (0, 0, 30) looking along -z: the oracle's primary frame hits 1 008 of the 2 304 pixels on 994 distinct
    triangles with ids 4 979 .. 1 047 997 (CPU), so the gather reads all over the snapshot — but not its last group of 64 triangles, the ragged one, which
    holds the two outliers alone: after the pose two more cameras look at those.  The filtered image is not compared: tests/test_gpu_denoise_motion.py holds it against numpy, and nothing in the merge depends on the triangle count."""
    n = TOP
    c, tris = case(n), S.far_ends(n)
    b, woop = S.host_tree(n, "linear")
    ip, iv = api.camera_matrices(60.0, 0.0, 0.0, W, H)
    pos = np.array(CAMERA, np.float32)
    # the oracle's primary frame of the rest pose
    k = api.InstanceConfig().c
    prm = O.make_params(W, H, list(CAMERA), ip, iv, stack_size=PT["stack_size"], max_bounce=PT["max_bounce"], subpixel=1, tmp_life=PT["tmp_life"], tmin=k.ray_tmin, clamp=k.clamp,
                        sun=list(k.sun))
    want_tri = O.primary_frame(O.Scene(b.nodes, b.tri_indices, tris, c.scene.materials, woop=woop), prm, 0)[1]["tri_id"]
    hs = api.HipScene()
    hs.Initialize(c.scene, b)
    p = api.HipPathTracer()
    cfg = params()
    cfg.subpixel = 1
    p.Initialize(cfg, hs, W, H)
    p.SetNoiseStats(True)
    p.SetCamera(ip, iv, pos)
    p.Trace(True, 2)
    tri, _ = p.ReadHits()
    ids = tri[tri >= 0]
    print("hit pixels %d of %d, distinct triangles %d, ids %d .. %d" % (len(ids), tri.size, len(np.unique(ids)), ids.min(), ids.max()))
    assert len(ids) >= 900 and len(np.unique(ids)) >= 800 and ids.min() < n // 2 < ids.max()
    assert np.array_equal(tri, want_tri), "the primary hits are not the oracle's"
    assert p.GetDenoiseMotion()["have_snapshot"] == 0
    p.Denoise(temporal=True, follow_motion=True)  # commits: the snapshot of all n triangles
    info = p.GetDenoiseMotion()
    assert info["have_snapshot"] == 1 and info["n_tris"] == n and info["device_bytes"] >= 80 * n + 32 * W * H and info["snapshot_ms"] > 0.0
    assert not p.ReadDenoiseMotion()["moved"].any()
    # every triangle moves
    mats, parts = gentle(N_MATRICES), P.parts_of(n, N_MATRICES)
    assert not any(np.array_equal(m, P.identity()) for m in mats)
    posed = host_posed(tris, mats, parts=parts)
    p.BindParts(parts, N_MATRICES)
    p.Pose(mats)
    posed_nodes, posed_woop = refit_of(n, "linear", posed, "parts")
    posed_scene = O.Scene(posed_nodes, b.tri_indices, posed, c.scene.materials, woop=posed_woop)
    rest_words, posed_words = TM.tri_words(tris["p"], tris["n"]), TM.tri_words(posed["p"], posed["n"])
    # The camera of before; then one 2 in front of each of the last two triangles, which that camera does not see (they are the last group of the
    # snapshot's kernel, the ragged one): (position, the triangle to be seen or None, the least hit pixels).  On the CPU the oracle's frames hit 1 553, 397 and
    # 7 pixels, 13 and 7 of them on the triangle in front
    cameras = [(CAMERA, None, 900)] + [(tuple(posed["p"][i].astype(np.float64).mean(axis=0) + (0.0, 0.0, 2.0)), i, 5) for i in (n - 2, n - 1)]
    for at, must_see, least in cameras:
        p.Reset()
        p.SetCamera(ip, iv, np.array(at, np.float32))
        p.Trace(True, 2)
        tri, uv = p.ReadHits()
        hit = tri >= 0
        print("after the pose, camera at %s: hit pixels %d, on triangle %s %d" % (at, hit.sum(), must_see, (tri == must_see).sum() if must_see is not None else 0))
        prm.origin[:] = [float(np.float32(x)) for x in at]
        assert np.array_equal(tri, O.primary_frame(posed_scene, prm, 0)[1]["tri_id"]), "the primary hits of the posed scene"
        assert hit.sum() >= least and (must_see is None or (tri == must_see).sum() >= 5)
        p.Denoise(temporal=True, follow_motion=True, commit=False)
        m, g = p.ReadDenoiseMotion(), p.ReadDenoiseGuides()
        assert np.array_equal(m["moved"], hit), "moved is not exactly the pixels that hit a triangle"
        want = TM.previous_point(rest_words, posed_words, tri, uv, g["normal"], g["position"])[0]
        assert np.array_equal(bits(m["previous_position"][hit]), bits(want[hit])), "the previous position of the moved pixels"
        assert not np.array_equal(bits(want[hit]), bits(g["position"][hit]))
        info = p.GetDenoiseMotion()
        assert info["have_snapshot"] == 1 and info["n_tris"] == n
    p.destroy()
