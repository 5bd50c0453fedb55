"""-m gpu: morph targets on the device (include/adypt_hip.h adypt_bind_morph, adypt_pose_morph; k_pose<., true> in csrc/device/pose.hip).  The device's
triangle records after Pose(mats, morph_weights=w) are held against the host's adypt_pose_triangles_morph packed by tests/tri_record_truth.py byte for
byte (and that function against numpy in tests/test_morph_definition.py); nodes and Woop data against adypt_bvh_refit + adypt_woop_matrices of the
host-posed triangles; images against the CPU oracle, bit for bit.  A workgroup of k_pose takes 256 triangles: the scenes have 1, 255, 256, 257 and
5 000.  The layers are tests/morph_truth.entries_of: triangle 0 without an entry, the last one with entries (the offset at n is read), neighbours with
0, 1, 2, 12 and n_targets entries (the loop diverges), weights of 0 between active ones on one triangle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import morph_truth as M  # noqa: E402
from tests import pose_truth as P  # noqa: E402
from tests import refit_truth as T  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_gpu_pose import bind, binding_of, expect_tree, gentle, records_of, same_state, small, state, with_zero  # noqa: E402
from tests.test_gpu_refit import SPP, case_of, oracle_image, tracer  # noqa: E402
from tests.test_refit_definition import lib_refit, same_bytes  # noqa: E402


def host_posed(tris, mats, entries=None, w=None, **binding):
    t = api.pose_triangles(tris, mats, morph=entries, morph_weights=w, **binding).view(O.TRI_DT)
    t.setflags(write=False)
    return t


def usable(binding):
    """skin weights under which every triangle stays one: no vertex without a joint"""
    if "weights" in binding:
        none = (binding["weights"] == 0).all(axis=-1)
        binding["weights"][none, 0], binding["joints"][none, 0] = 1.0, 1
    return binding


def identities(nm):
    return np.stack([P.identity()] * nm)


# ---- 1. records ----
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_records_equal_the_host_definition(n, scene_cache):
    case = case_of("soup", scene_cache) if n == 5000 else small(n)
    p = tracer(case, case.scene, case.bvh(48))
    rest = p.ReadTriangleRecords()
    assert p.GetMorphBinding() == {"n_targets": 0, "n_entries": 0, "n_tris_touched": 0, "device_bytes": 0}
    for kind in ("parts", "skin"):
        nm = 3
        mats, binding = with_zero(nm), binding_of(kind, n, nm)
        p.UpdateTriangles(0, case.tris["p"].reshape(-1, 9), case.tris["n"].reshape(-1, 9))  # (a bind captures the records as they are: the rest pose again)
        bind(p, binding, nm)
        for nt in (1, 3, 300):
            entries, w = M.entries_of(n, nt), M.weights_of(nt)
            count = np.bincount(entries[0], minlength=n)
            assert count[n - 1] > 0 and (n < 5 or (count[:5] == (0, 1, min(nt, 2), min(nt, 12), nt)).all())
            p.BindMorph(*entries, nt)
            got = p.GetMorphBinding()
            assert (got["n_targets"], got["n_entries"], got["n_tris_touched"]) == (nt, len(entries[0]), int((count > 0).sum()))
            assert got["device_bytes"] >= 76 * len(entries[0]) + 4 * (n + 1) + 4 * nt
            assert p.Pose(mats, morph_weights=w) is None
            want = records_of(case, host_posed(case.tris, mats, entries, w, **binding))
            rec = p.ReadTriangleRecords()
            assert rec.tobytes() == want.tobytes(), (kind, nt)
            assert np.array_equal(rec[:, 18:], rest[:, 18:])  # material id, class word, texture coordinates, zeros: their bytes
            assert rec.tobytes() != records_of(case, host_posed(case.tris, mats, **binding)).tobytes()
    p.destroy()


# ---- 2. no layer, or all weights 0 ----
@pytest.mark.parametrize("kind", ["parts", "skin"])
def test_zero_weights_equal_a_tracer_without_a_layer(kind, scene_cache):
    case = small(257)
    n, nm, nt = 257, 4, 3
    mats, binding, entries = gentle(nm), usable(binding_of(kind, n, nm)), M.entries_of(n, nt)
    with_layer, without = tracer(case, case.scene, case.bvh()), tracer(case, case.scene, case.bvh())
    for p in (with_layer, without):
        bind(p, binding, nm)
    with_layer.BindMorph(*entries, nt)
    without.Pose(mats)
    want = state(without)
    with_layer.Pose(mats, morph_weights=M.weights_of(nt))
    assert not same_state(state(with_layer), want)
    with_layer.Pose(mats)
    assert same_state(state(with_layer), want), "Pose(mats) on a binding with a layer"
    with_layer.Pose(mats, morph_weights=M.weights_of(nt))
    with_layer.Pose(mats, morph_weights=np.zeros(nt, np.float32))
    assert same_state(state(with_layer), want), "all weights 0"
    # a weight of 0 and deltas of 3e38: never read
    huge = entries[2].copy()
    huge[entries[1] == 1] = 3e38
    w = M.weights_of(nt)
    assert w[1] == 0
    with_layer.BindMorph(entries[0], entries[1], huge, nt)
    with_layer.Pose(mats, morph_weights=w)
    assert with_layer.ReadTriangleRecords().tobytes() == records_of(case, host_posed(case.tris, mats, entries, w, **binding)).tobytes()
    with_layer.destroy()
    without.destroy()


# ---- 3. tree and image ----
@pytest.mark.parametrize("name,kind", [("tiny0", "parts"), ("soup", "skin")])
def test_tree_and_image_after_a_morph_pose(name, kind, scene_cache, sobol_matrices):
    case = case_of(name, scene_cache)
    b, n, nm, nt = case.bvh(48), len(case.tris), 6, 3
    mats, binding = gentle(nm), usable(binding_of(kind, n, nm))
    entries, w = M.entries_of(n, nt), M.weights_of(nt)
    posed, unmorphed = host_posed(case.tris, mats, entries, w, **binding), host_posed(case.tris, mats, **binding)
    p = tracer(case, case.scene, b)
    p.Trace(True, 2)  # (the rest pose has been rendered: per-reference records, primary-hit cache and image are its)
    bind(p, binding, nm)
    p.BindMorph(*entries, nt)
    p.Pose(mats, morph_weights=w)
    assert p.GetSPP() == 0
    want_nodes = expect_tree(p, b, posed)
    plain_nodes = host_refit_of(b, unmorphed)
    assert not same_bytes(want_nodes, plain_nodes)
    p.Trace(True, SPP)
    want = oracle_image(case, want_nodes, b.tri_indices, posed, sobol_matrices)
    assert np.array_equal(bits(p.ReadResult()), bits(want)), "the image of the morphed and posed scene"
    assert not np.array_equal(bits(want), bits(oracle_image(case, plain_nodes, b.tri_indices, unmorphed, sobol_matrices)))  # the layer shows
    p.destroy()


def host_refit_of(b, posed):
    r, nodes = lib_refit(b.nodes, b.tri_indices, posed)
    assert r == N.ADYPT_OK
    return nodes


# ---- 4. no compounding ----
def test_morph_poses_do_not_compound(scene_cache):
    case = case_of("soup", scene_cache)
    n, nm, nt = len(case.tris), 5, 3
    binding, entries = binding_of("parts", n, nm), M.entries_of(n, nt)
    A, B = gentle(nm), np.ascontiguousarray(gentle(nm)[::-1])
    wA, wB = M.weights_of(nt), np.array([0.5, -1.25, 0.0], np.float32)
    twice, once = tracer(case, case.scene, case.bvh(48)), tracer(case, case.scene, case.bvh(48))
    for p in (twice, once):
        bind(p, binding, nm)
        p.BindMorph(*entries, nt)
    twice.Pose(A, morph_weights=wA)
    twice.Pose(B, morph_weights=wB)
    once.Pose(B, morph_weights=wB)
    assert same_state(state(twice), state(once))
    assert twice.ReadTriangleRecords().tobytes() == records_of(case, host_posed(case.tris, B, entries, wB, **binding)).tobytes()
    once.destroy()
    twice.destroy()


# ---- 5. refusals ----
def test_refusals_change_nothing(scene_cache):
    case = case_of("tiny0", scene_cache)
    n, nm, nt = len(case.tris), 4, 3
    parts, mats = P.parts_of(n, nm), gentle(nm)
    tri, tgt, d = M.entries_of(n, nt)
    w = M.weights_of(nt)
    p = tracer(case, case.scene, case.bvh(48))
    c = p._ctx
    # no binding yet
    with pytest.raises(N.AdyptError) as e:
        p.BindMorph(tri, tgt, d, nt)
    assert e.value.code == N.E_STATE and p.GetMorphBinding()["n_targets"] == 0
    p.BindParts(parts, nm)
    # weights without a layer
    with pytest.raises(N.AdyptError) as e:
        p.Pose(mats, morph_weights=w)
    assert e.value.code == N.E_INVALID
    p.BindMorph(tri, tgt, d, nt)
    layer = p.GetMorphBinding()
    p.Pose(mats, morph_weights=w)
    before = state(p)
    p.Trace(True, SPP)
    image = p.ReadResult()
    flat = np.ascontiguousarray(mats.reshape(-1, 12))
    ne = len(tri)

    def bad(a, at, value):
        a = a.copy()
        a[at] = value
        return a

    refusals = [
        ("triangles is null", lambda: N.lib.adypt_bind_morph(c, None, tgt.ctypes.data, d.ctypes.data, ne, nt)),
        ("targets is null", lambda: N.lib.adypt_bind_morph(c, tri.ctypes.data, None, d.ctypes.data, ne, nt)),
        ("deltas is null", lambda: N.lib.adypt_bind_morph(c, tri.ctypes.data, tgt.ctypes.data, None, ne, nt)),
        ("weights is null", lambda: N.lib.adypt_pose_morph(c, flat.ctypes.data, nm, None, nt, None, None, None)),
        ("matrices is null", lambda: N.lib.adypt_pose_morph(c, None, nm, w.ctypes.data, nt, None, None, None)),
        ("no entries", lambda: N.lib.adypt_bind_morph(c, tri.ctypes.data, tgt.ctypes.data, d.ctypes.data, 0, nt)),
        ("a negative entry count", lambda: N.lib.adypt_bind_morph(c, tri.ctypes.data, tgt.ctypes.data, d.ctypes.data, -1, nt)),
        ("too many entries", lambda: N.lib.adypt_bind_morph(c, tri.ctypes.data, tgt.ctypes.data, d.ctypes.data, 2 ** 31, nt)),
        ("no targets", lambda: p.BindMorph(tri, tgt, d, 0)),
        ("too many targets", lambda: p.BindMorph(tri, tgt, d, 65537)),
        ("a triangle below 0", lambda: p.BindMorph(bad(tri, 3, -1), tgt, d, nt)),
        ("a triangle past the last", lambda: p.BindMorph(bad(tri, ne - 1, n), tgt, d, nt)),
        ("a target below 0", lambda: p.BindMorph(tri, bad(tgt, 0, -1), d, nt)),
        ("a target past the last", lambda: p.BindMorph(tri, bad(tgt, ne // 2, nt), d, nt)),
        ("an infinite delta", lambda: p.BindMorph(tri, tgt, bad(d, (2, 17), np.inf), nt)),
        ("a NaN delta", lambda: p.BindMorph(tri, tgt, bad(d, (ne - 1, 0), np.nan), nt)),
        ("two entries of one triangle and target", lambda: p.BindMorph(np.append(tri, tri[5]), np.append(tgt, tgt[5]), np.concatenate([d, d[5:6]]), nt)),
        ("fewer weights", lambda: p.Pose(mats, morph_weights=w[:-1])),
        ("more weights", lambda: p.Pose(mats, morph_weights=np.append(w, 1.0))),
        ("an infinite weight", lambda: p.Pose(mats, morph_weights=bad(w, 0, np.inf))),
        ("a NaN weight", lambda: p.Pose(mats, morph_weights=bad(w, 2, np.nan))),
        ("fewer matrices", lambda: p.Pose(mats[:-1], morph_weights=w)),
        ("a NaN matrix entry", lambda: p.Pose(bad(mats, (3, 0, 0), np.nan), morph_weights=w)),
        ("a negative threshold", lambda: p.Pose(mats, rebuild_above=-1.0, morph_weights=w)),
    ]
    for what, call in refusals:
        try:
            code = call()
        except N.AdyptError as err:
            code = err.code
        assert code == N.E_INVALID, what
        assert same_state(state(p), before), what
        assert p.GetSPP() == SPP and np.array_equal(bits(p.ReadResult()), bits(image)), what  # not even the accumulation
        assert p.GetMorphBinding() == layer and p.GetPoseBinding()["kind"] == 1, what
    # the refused binds have left the layer in place: the next pose is its
    other = np.array([1.0, 0.5, -0.5], np.float32)
    p.Pose(mats, morph_weights=other)
    assert p.ReadTriangleRecords().tobytes() == records_of(case, host_posed(case.tris, mats, (tri, tgt, d), other, parts=parts)).tobytes()
    p.destroy()


# ---- 6. lifetime ----
def test_layer_lifetime(scene_cache):
    case = case_of("soup", scene_cache)
    n, nm, nt = len(case.tris), 5, 3
    binding, A = binding_of("parts", n, nm), gentle(nm)
    entries, w = M.entries_of(n, nt), M.weights_of(nt)
    posed = host_posed(case.tris, A, entries, w, **binding)
    plain = records_of(case, host_posed(case.tris, A, **binding)).tobytes()
    p = tracer(case, case.scene, case.bvh(48))
    bind(p, binding, nm)
    pose_binding = p.GetPoseBinding()
    p.BindMorph(*entries, nt)
    assert p.GetPoseBinding() == pose_binding and set(pose_binding) == {"kind", "n_matrices", "n_tris", "device_bytes"}
    assert p.GetMorphBinding()["device_bytes"] >= 76 * len(entries[0]) + 4 * (n + 1) + 4 * nt
    # a rebuild keeps the layer: the pose refits the rebuilt tree
    p.RebuildBVH(method="ploc")
    built = api.WideBVH()
    built.nodes, built.tri_indices = p.ReadBVH()[0], p.ReadTriIndices()
    assert p.GetMorphBinding()["n_targets"] == nt
    p.Pose(A, morph_weights=w)
    expect_tree(p, built, posed, "after a rebuild")
    # an update writes the posed records: neither the rest pose nor the layer
    moved = T.wave(case.tris)
    p.UpdateTriangles(0, moved["p"].reshape(-1, 9))
    assert p.GetMorphBinding()["n_targets"] == nt
    p.Pose(A, morph_weights=w)
    assert p.ReadTriangleRecords().tobytes() == records_of(case, posed).tobytes()
    # UnbindMorph leaves the matrix binding
    p.UnbindMorph()
    assert p.GetMorphBinding() == {"n_targets": 0, "n_entries": 0, "n_tris_touched": 0, "device_bytes": 0} and p.GetPoseBinding() == pose_binding
    p.Pose(A)
    assert p.ReadTriangleRecords().tobytes() == plain
    # a new bind of the matrices captures a new rest pose: the layer goes
    p.UpdateTriangles(0, case.tris["p"].reshape(-1, 9), case.tris["n"].reshape(-1, 9))
    p.BindMorph(*entries, nt)
    bind(p, binding, nm)
    assert p.GetMorphBinding()["n_targets"] == 0
    p.Pose(A)
    assert p.ReadTriangleRecords().tobytes() == plain
    # UnbindPose and SetTriangles drop it too
    p.BindMorph(*entries, nt)
    p.UnbindPose()
    assert p.GetMorphBinding()["n_targets"] == 0 and p.GetPoseBinding()["kind"] == 0
    p.UpdateTriangles(0, case.tris["p"].reshape(-1, 9), case.tris["n"].reshape(-1, 9))
    bind(p, binding, nm)
    p.BindMorph(*entries, nt)
    p.SetTriangles(case.scene.triangles)
    assert p.GetMorphBinding()["n_targets"] == 0
    with pytest.raises(N.AdyptError) as e:
        p.BindMorph(*entries, nt)
    assert e.value.code == N.E_STATE
    p.destroy()


# ---- 7. policy ----
def test_morph_pose_under_a_policy(scene_cache):
    case = case_of("soup", scene_cache)
    n, nm, nt = len(case.tris), 5, 3
    binding, A = binding_of("parts", n, nm), gentle(nm)
    entries, w = M.entries_of(n, nt), M.weights_of(nt)
    b = case.bvh(48)
    auto, plain, kept = (tracer(case, case.scene, b) for _ in range(3))
    for p in (auto, plain, kept):
        bind(p, binding, nm)
        p.BindMorph(*entries, nt)
    out = auto.Pose(A, morph_weights=w, rebuild_above=0)
    plain.Pose(A, morph_weights=w)
    refit_nodes = plain.ReadBVH()[0]
    plain.RebuildBVH(method="ploc")
    assert out["rebuilt"] == 1
    assert same_state(state(auto), state(plain)) and np.array_equal(auto.ReadTriIndices(), plain.ReadTriIndices())
    out = kept.Pose(A, morph_weights=w, rebuild_above=1e9)
    assert out["rebuilt"] == 0 and out["now"] == out["refitted"]
    assert same_bytes(kept.ReadBVH()[0], refit_nodes) and np.array_equal(kept.ReadTriIndices(), b.tri_indices)
    assert kept.ReadTriangleRecords().tobytes() == records_of(case, host_posed(case.tris, A, entries, w, **binding)).tobytes()
    for p in (auto, plain, kept):
        p.destroy()


# ---- 8. several shards on one card ----
def test_two_shards_on_one_device(scene_cache, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = case_of("soup", scene_cache)
    n, nm, nt = len(case.tris), 5, 3
    A, binding = gentle(nm), usable(binding_of("skin", n, nm))
    entries, w = M.entries_of(n, nt), M.weights_of(nt)
    wd, h = 64, 36  # 2 x 2 blocks: both shards own some
    single = tracer(case, case.scene, case.bvh(48), wd, h)
    multi = tracer(case, case.scene, case.bvh(48), wd, h, cls=api.MultiPathTracer, devices=(0, 0))
    assert multi.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in multi._contexts())
    for t in (single, multi):
        t.Trace(True, 2)
        bind(t, binding, nm)
        t.BindMorph(*entries, nt)
        t.Pose(A, morph_weights=w)
        assert t.GetSPP() == 0
        t.Trace(True, SPP)
    a = single.ReadBVH()
    for c in multi._contexts():  # every device posed its own copy
        nodes, woop = np.zeros_like(a[0]), np.zeros_like(a[1])
        N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, woop.ctypes.data), c)
        assert same_bytes(nodes, a[0]) and np.array_equal(bits(woop), bits(a[1]))
    assert multi.GetMorphBinding() == single.GetMorphBinding() and multi.GetMorphBinding()["n_targets"] == nt
    assert np.array_equal(bits(multi.ReadResult()), bits(single.ReadResult()))
    assert not np.array_equal(bits(single.ReadResult()), np.zeros_like(bits(single.ReadResult())))
    for call in (lambda: multi.Pose(A, morph_weights=w[:-1]), lambda: multi.BindMorph(entries[0], entries[1] + nt, entries[2], nt)):
        with pytest.raises(N.AdyptError) as e:
            call()
        assert e.value.code == N.E_INVALID
    assert multi.GetMorphBinding() == single.GetMorphBinding()
    multi.UnbindMorph()
    assert multi.GetMorphBinding()["n_targets"] == 0 and multi.GetPoseBinding() == single.GetPoseBinding()
    multi.destroy()
    single.destroy()


# ---- 9. the temporal merge follows a morph ----
def test_temporal_merge_follows_a_morph(scene_cache, sobol_matrices):
    from tests import temporal_motion_truth as TM
    from tests import test_gpu_denoise_motion as DM
    from tests.test_gpu_denoise_temporal import GEOMETRY, SEED, camera_of, oracle_pose

    inst, _, tris, on_box = DM.instance(scene_cache)
    p, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    n, box = len(tris), np.nonzero(on_box)[0].astype(np.int32)
    # two targets on the 12 triangles of the box: one moves it, one shears it upwards
    tri, tgt = np.concatenate([box, box]), np.repeat(np.array([0, 1], np.int32), len(box))
    d = np.zeros((len(tri), 2, 3, 3), np.float32)
    d[: len(box), 0] = (0.3, 0.3, 0.3)
    d[len(box):, 0] = (tris["p"][box] - np.array([-1.5, 0.0, 1.3], np.float32)) * np.array([0.0, 0.4, 0.0], np.float32) + np.array([-0.2, 0.0, 0.1], np.float32)
    entries = (tri, tgt, d.reshape(-1, 18))
    wA, wB = np.array([1.0, 0.0], np.float32), np.array([0.5, 1.0], np.float32)
    parts, eye = np.zeros(n, np.int32), identities(1)
    trisA, trisB = (np.array(host_posed(tris, eye, entries, w, parts=parts)) for w in (wA, wB))

    def oracle_of(key, t, k, seed):
        b = api.WideBVH()
        b.BuildPLOC(api.Scene.FromArrays(t, inst.scene.materials), cfg.bvh_params(), 8, 0.0)
        osc = O.Scene(b.nodes, b.tri_indices, np.ascontiguousarray(t).view(np.uint8).reshape(-1), inst.scene.materials, textures=inst.scene.textures)
        pos, yaw = camera_of(c, GEOMETRY[0], k)
        call, cam, _, hit_tri = oracle_pose(key, osc, c, pos, yaw, seed, sobol_matrices)
        ip, iv = O.camera(c.fov, yaw, c.pitch, c.width, c.height)
        prm = O.make_params(c.width, c.height, pos, ip, iv, stack_size=c.stack_size, max_bounce=c.max_bounce, subpixel=c.subpixel, tmp_life=c.tmp_lifetime, tmin=c.ray_tmin,
                            clamp=c.clamp, sun=list(c.sun))
        hits = O.primary_frame(osc, prm, 0)[1]
        return dict(pos=pos, yaw=yaw, seed=seed, call=call, cam=cam, tri=hit_tri, uv=np.stack([hits["u"], hits["v"]], -1).astype(np.float32))

    A, B = oracle_of(("morph", "A"), trisA, 0, SEED), oracle_of(("morph", "B"), trisB, 1, SEED + 1)
    wantA = TM.denoise(*A["call"], None, A["cam"], A["tri"], A["uv"], DM.words(trisA))
    wantB = TM.denoise(*B["call"], wantA[2], B["cam"], B["tri"], B["uv"], DM.words(trisB))
    changed = np.nonzero((bits(DM.words(trisA)) != bits(DM.words(trisB))).reshape(n, -1).any(axis=1))[0]
    assert np.array_equal(changed, box)
    on_changed = np.isin(B["tri"], changed)
    assert on_changed.sum() > 50

    p.BindParts(parts, 1)
    p.BindMorph(*entries, 2)
    p.Pose(eye, morph_weights=wA)
    DM.go(p, cfg, A)
    DM.assert_truth(DM.motion_call(p), wantA, "morph A")
    p.Pose(eye, morph_weights=wB)
    DM.go(p, cfg, B)
    got = DM.motion_call(p)
    DM.assert_truth(got, wantB, "morph B")
    assert np.array_equal(got[3], on_changed), "moved is not exactly the pixels whose primary hit lies on a triangle whose record changed"
    p.destroy()


# ---- 10. timing ----
def test_refit_timing_answers_after_a_morph_pose(scene_cache):
    case = small(257)
    p = tracer(case, case.scene, case.bvh())
    p.BindParts(P.parts_of(257, 3), 3)
    p.BindMorph(*M.entries_of(257, 3), 3)
    p.Pose(gentle(3), morph_weights=M.weights_of(3))
    ms = p.GetRefitTiming()
    assert set(ms) == {"scatter", "references_woop", "nodes", "total"}
    assert all(np.isfinite(v) and v >= 0.0 for v in ms.values()) and ms["total"] > 0.0 and ms["scatter"] > 0.0
    p.destroy()
