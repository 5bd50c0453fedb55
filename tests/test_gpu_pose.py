"""-m gpu: posing on the device (include/adypt_hip.h adypt_bind_parts, adypt_bind_skin, adypt_pose; csrc/device/pose.hip).  The device's triangle
records after a pose are held against the host's adypt_pose_triangles packed by tests/tri_record_truth.py byte for byte (and that function against
numpy in tests/test_pose_definition.py); nodes and Woop data against adypt_bvh_refit + adypt_woop_matrices of the host-posed triangles; images against
the CPU oracle on those arrays, bit for bit.  A workgroup of k_pose takes 256 triangles: the scenes have 1, 255, 256, 257 and 5 000."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import pose_truth as P  # noqa: E402
from tests import refit_truth as T  # noqa: E402
from tests import tri_record_truth as R  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_gpu_refit import SPP, case_of, oracle_image, same_woop, tracer  # noqa: E402
from tests.test_refit_definition import lib_refit, same_bytes  # noqa: E402

_small = {}


class Small:
    """what tracer() asks of a case, for a soup of n triangles: texture coordinates and material ids (0, and -1 on every third) that a pose must keep"""

    def __init__(self, n):
        self.tris = T.soup(n, 3)
        self.tris["tc"] = np.random.RandomState(n).uniform(size=self.tris["tc"].shape).astype(np.float32)
        self.tris["matid"] = np.where(np.arange(n) % 3 == 2, -1, 0)
        self.tris.setflags(write=False)
        self.scene = api.Scene.FromArrays(self.tris, T.soup_material())
        self.ip, self.iv = api.camera_matrices(60.0, 30.0, -10.0, 32, 18)
        self.pos = np.zeros(3, np.float32)
        self._b = None

    def bvh(self, depth=48):
        if self._b is None:
            self._b = api.WideBVH()
            self._b.Build(self.scene, api.InstanceConfig().bvh_params())
            self._b.nodes.setflags(write=False)
        return self._b


def small(n):
    if n not in _small:
        _small[n] = Small(n)
    return _small[n]


def with_zero(nm):
    """nm matrices; from three on, index 2 is the zero matrix"""
    m = P.matrix_set(max(nm, 4))
    m[[2, 3]] = m[[3, 2]]
    return np.ascontiguousarray(m[:nm])


def gentle(nm):
    """nm matrices that leave every triangle a triangle: a rotation, a non-uniform scale, a mirror, random affine maps"""
    return np.ascontiguousarray(np.delete(P.matrix_set(nm + 1), 3, axis=0)[:nm])


def host_posed(tris, mats, **binding):
    t = api.pose_triangles(tris, mats, **binding).view(O.TRI_DT)
    t.setflags(write=False)
    return t


def records_of(case, tris):
    return R.pack(tris, case.scene.materials, len(case.scene.textures))[0]


def bind(p, binding, nm):
    if "parts" in binding:
        p.BindParts(binding["parts"], nm)
    else:
        p.BindSkin(binding["joints"], binding["weights"], nm)


def binding_of(kind, n, nm):
    if kind == "parts":
        return {"parts": P.parts_of(n, nm)}
    j, w = P.skin_of(n, nm)
    return {"joints": j, "weights": w}


def state(p):
    nodes, woop = p.ReadBVH()
    return p.ReadTriangleRecords(), nodes, woop


def same_state(a, b):
    return a[0].tobytes() == b[0].tobytes() and same_bytes(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))  # (device against device: NaNs included)


def expect_tree(p, b, posed, what=""):
    nodes, woop = p.ReadBVH()
    r, want = lib_refit(b.nodes, b.tri_indices, posed)
    assert r == N.ADYPT_OK
    assert same_bytes(nodes, want), "nodes " + what
    assert same_woop(woop, api.woop_matrices(posed, b.tri_indices)), "Woop data " + what
    return want


# ---- 1. records ----
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_records_equal_the_host_definition(n, scene_cache):
    case = case_of("soup", scene_cache) if n == 5000 else small(n)
    p = tracer(case, case.scene, case.bvh(48))
    rest = p.ReadTriangleRecords()
    assert rest.tobytes() == records_of(case, case.tris).tobytes()
    assert p.GetPoseBinding() == {"kind": 0, "n_matrices": 0, "n_tris": 0, "device_bytes": 0}
    for kind in ("parts", "skin"):
        for nm in (1, 3, 300):
            mats, binding = with_zero(nm), binding_of(kind, n, nm)
            p.UpdateTriangles(0, case.tris["p"].reshape(-1, 9), case.tris["n"].reshape(-1, 9))  # (a bind captures the records as they are: the rest pose again)
            bind(p, binding, nm)
            got = p.GetPoseBinding()
            assert (got["kind"], got["n_matrices"], got["n_tris"]) == (1 if kind == "parts" else 2, nm, n)
            assert got["device_bytes"] >= n * (76 if kind == "parts" else 144) + 48 * nm
            assert p.Pose(mats) is None
            posed = host_posed(case.tris, mats, **binding)
            want = records_of(case, posed)
            rec = p.ReadTriangleRecords()
            assert rec.tobytes() == want.tobytes(), (kind, nm)
            assert np.array_equal(rec[:, 18:], rest[:, 18:])  # material id, class word, texture coordinates, zeros: their bytes
            if nm >= 3 and n >= 3:
                assert not np.array_equal(rec[:, :18], rest[:, :18])
    p.UnbindPose()
    assert p.GetPoseBinding()["kind"] == 0
    p.destroy()


# ---- 2. tree and image ----
@pytest.mark.parametrize("kind", ["parts", "skin"])
@pytest.mark.parametrize("name", ["tiny0", "soup"])
def test_tree_and_image_after_a_pose(name, kind, scene_cache, sobol_matrices):
    case = case_of(name, scene_cache)
    b, n, nm = case.bvh(48), len(case.tris), 6
    mats, binding = gentle(nm), binding_of(kind, n, nm)
    if kind == "skin":  # (weights that sum to 1, no vertex without a joint: every triangle stays one)
        none = (binding["weights"] == 0).all(axis=-1)
        binding["weights"][none, 0], binding["joints"][none, 0] = 1.0, 1
    posed = host_posed(case.tris, mats, **binding)
    p = tracer(case, case.scene, b)
    p.Trace(True, 2)  # (the rest pose has been rendered: per-reference records, primary-hit cache and image are its)
    bind(p, binding, nm)
    p.Pose(mats)
    assert p.GetSPP() == 0
    want_nodes = expect_tree(p, b, posed)
    assert not same_bytes(want_nodes, b.nodes)
    p.Trace(True, SPP)
    want = oracle_image(case, want_nodes, b.tri_indices, posed, sobol_matrices)
    assert np.array_equal(bits(p.ReadResult()), bits(want)), "the image of the posed scene"
    assert not np.array_equal(bits(want), bits(oracle_image(case, b.nodes, b.tri_indices, case.tris, sobol_matrices)))  # the pose shows
    p.destroy()


# ---- 3. no compounding ----
def test_poses_do_not_compound(scene_cache):
    case = case_of("soup", scene_cache)
    n, nm = len(case.tris), 5
    binding = binding_of("parts", n, nm)
    A, B = gentle(nm), np.ascontiguousarray(gentle(nm)[::-1])
    twice, once = tracer(case, case.scene, case.bvh(48)), tracer(case, case.scene, case.bvh(48))
    for p in (twice, once):
        bind(p, binding, nm)
    twice.Pose(A)
    twice.Pose(B)
    once.Pose(B)
    assert same_state(state(twice), state(once))
    assert twice.ReadTriangleRecords().tobytes() == records_of(case, host_posed(case.tris, B, **binding)).tobytes()
    once.destroy()
    twice.Pose(A)
    twice.Pose(np.stack([P.identity()] * nm))
    rec, rest = twice.ReadTriangleRecords(), records_of(case, case.tris)
    assert np.array_equal(rec[:, :9].view(np.float32), rest[:, :9].view(np.float32))  # as numbers: x * 1 + y * 0 + z * 0 + 0
    twice.destroy()


# ---- 4. parts against skin ----
def test_parts_equal_skin_of_one_full_weight(scene_cache):
    case = small(257)
    n, nm = len(case.tris), 3
    parts, mats = P.parts_of(n, nm), with_zero(nm)
    joints = np.full((n, 3, 4), 65535, dtype=np.uint16)  # garbage in the slots of weight 0
    joints[..., 1] = parts[:, None]
    weights = np.zeros((n, 3, 4), dtype=np.float32)
    weights[..., 1] = 1.0
    a, b = tracer(case, case.scene, case.bvh()), tracer(case, case.scene, case.bvh())
    a.BindParts(parts, nm)
    b.BindSkin(joints, weights, nm)
    a.Pose(mats)
    b.Pose(mats)
    assert a.ReadTriangleRecords().tobytes() == b.ReadTriangleRecords().tobytes()
    assert same_state(state(a), state(b))
    a.destroy()
    b.destroy()


# ---- 5. refusals ----
def test_refusals_change_nothing(scene_cache):
    case = case_of("tiny0", scene_cache)
    n, nm = len(case.tris), 4
    parts, mats = P.parts_of(n, nm), gentle(nm)
    joints, weights = P.skin_of(n, nm)
    p = tracer(case, case.scene, case.bvh(48))
    c = p._ctx
    # no binding yet
    with pytest.raises(N.AdyptError) as e:
        p.Pose(mats)
    assert e.value.code == N.E_STATE
    p.BindParts(parts, nm)
    p.Pose(mats)
    before = state(p)
    p.Trace(True, SPP)
    image = p.ReadResult()
    flat = np.ascontiguousarray(mats.reshape(-1, 12))
    j16, w32 = np.ascontiguousarray(joints.reshape(-1, 12)), np.ascontiguousarray(weights.reshape(-1, 12))

    def bad(a, at, value):
        a = a.copy()
        a[at] = value
        return a

    live = tuple(np.argwhere(weights != 0)[5])
    refusals = [
        ("parts is null", lambda: N.lib.adypt_bind_parts(c, None, n, nm)),
        ("joints is null", lambda: N.lib.adypt_bind_skin(c, None, w32.ctypes.data, n, nm)),
        ("weights is null", lambda: N.lib.adypt_bind_skin(c, j16.ctypes.data, None, n, nm)),
        ("matrices is null", lambda: N.lib.adypt_pose(c, None, nm, None, None, None)),
        ("fewer triangles", lambda: p.BindParts(parts[:-1], nm)),
        ("more triangles", lambda: p.BindSkin(np.concatenate([joints, joints[:1]]), np.concatenate([weights, weights[:1]]), nm)),
        ("no parts", lambda: p.BindParts(np.zeros(n, np.int32), 0)),
        ("too many parts", lambda: p.BindParts(parts, 65537)),
        ("no joints", lambda: p.BindSkin(joints, weights, 0)),
        ("too many joints", lambda: p.BindSkin(joints, weights, 65537)),
        ("a part below 0", lambda: p.BindParts(bad(parts, n // 2, -1), nm)),
        ("a part past the last", lambda: p.BindParts(bad(parts, n - 1, nm), nm)),
        ("a joint past the last", lambda: p.BindSkin(bad(joints, live, nm), weights, nm)),
        ("a negative weight", lambda: p.BindSkin(joints, bad(weights, live, -0.5), nm)),
        ("an infinite weight", lambda: p.BindSkin(joints, bad(weights, live, np.inf), nm)),
        ("a NaN weight", lambda: p.BindSkin(joints, bad(weights, live, np.nan), nm)),
        ("fewer matrices", lambda: p.Pose(mats[:-1])),
        ("more matrices", lambda: p.Pose(np.concatenate([mats, mats[:1]]))),
        ("an infinite matrix entry", lambda: p.Pose(bad(mats, (1, 2, 3), np.inf))),
        ("a NaN matrix entry", lambda: p.Pose(bad(mats, (3, 0, 0), np.nan))),
        ("a policy without a threshold", lambda: p.Pose(mats, rebuild_above=float("nan"))),
        ("a negative threshold", lambda: p.Pose(mats, rebuild_above=-1.0)),
        ("a radius out of range", lambda: p.Pose(mats, rebuild_above=0.0, radius=0)),
        ("a split budget out of range", lambda: p.Pose(mats, rebuild_above=0.0, split_budget=1.5)),
        ("a policy method out of range", lambda: N.lib.adypt_pose(c, flat.ctypes.data, nm, None, N.PosePolicy(1.0, 2, 8, 0.0), None)),
        ("SAH costs that are not positive", lambda: p.Pose(mats, rebuild_above=1.0, cfg=N.BvhParams(0, -1.0, 1.0))),
    ]
    for what, call in refusals:
        try:
            code = call()
        except N.AdyptError as err:
            code = err.code
        assert code == N.E_INVALID, what
        assert same_state(state(p), before), what
        assert p.GetSPP() == SPP and np.array_equal(bits(p.ReadResult()), bits(image)), what  # not even the accumulation
        assert p.GetPoseBinding()["kind"] == 1, what
    p.Reset()
    p.Trace(True, SPP)
    assert np.array_equal(bits(p.ReadResult()), bits(image))
    # the refused binds have left the parts binding in place: the next pose is its
    other = np.ascontiguousarray(mats[::-1])
    p.Pose(other)
    assert p.ReadTriangleRecords().tobytes() == records_of(case, host_posed(case.tris, other, parts=parts)).tobytes()
    p.destroy()


# ---- 6. lifetime ----
def test_binding_lives_through_rebuilds_and_updates(scene_cache):
    case = case_of("soup", scene_cache)
    n, nm = len(case.tris), 5
    binding, A, B = binding_of("parts", n, nm), gentle(nm), np.ascontiguousarray(gentle(nm)[::-1])
    p = tracer(case, case.scene, case.bvh(48))
    bind(p, binding, nm)
    # a rebuild keeps the binding: the pose refits the rebuilt tree
    p.RebuildBVH(method="ploc")
    built = api.WideBVH()
    built.nodes, built.tri_indices = p.ReadBVH()[0], p.ReadTriIndices()
    p.Pose(A)
    posed_a = host_posed(case.tris, A, **binding)
    expect_tree(p, built, posed_a, "after a rebuild")
    # a split tree loses its reference boxes to a pose as it does to an update
    p.RebuildBVH(method="ploc", split_budget=0.3)
    assert p.ReadRefBoxes() is not None
    p.Pose(A)
    assert p.ReadRefBoxes() is None
    assert p.ReadTriangleRecords().tobytes() == records_of(case, posed_a).tobytes()
    # an update writes the posed records, never the rest pose
    moved = T.wave(case.tris)
    p.UpdateTriangles(0, moved["p"].reshape(-1, 9))
    assert p.ReadTriangleRecords().tobytes() == records_of(case, _with_positions(posed_a, moved)).tobytes()
    p.Pose(B)
    assert p.ReadTriangleRecords().tobytes() == records_of(case, host_posed(case.tris, B, **binding)).tobytes()
    # a new bind captures the records as they are then
    p.UpdateTriangles(0, moved["p"].reshape(-1, 9), moved["n"].reshape(-1, 9))
    bind(p, binding, nm)
    p.Pose(A)
    assert p.ReadTriangleRecords().tobytes() == records_of(case, host_posed(moved, A, **binding)).tobytes()
    # new triangles drop the binding
    p.SetTriangles(case.scene.triangles)
    assert p.GetPoseBinding()["kind"] == 0
    with pytest.raises(N.AdyptError) as e:
        p.Pose(A)
    assert e.value.code == N.E_STATE
    p.destroy()


def _with_positions(tris, moved):
    t = np.array(tris)
    t["p"] = moved["p"]
    return t


# ---- 7. policy ----
def test_pose_under_a_policy(scene_cache):
    case = case_of("soup", scene_cache)
    n, nm = len(case.tris), 5
    binding, A = binding_of("parts", n, nm), gentle(nm)
    b = case.bvh(48)
    auto, plain, kept = (tracer(case, case.scene, b) for _ in range(3))
    for p in (auto, plain, kept):
        bind(p, binding, nm)
    out = auto.Pose(A, rebuild_above=0)
    plain.Pose(A)
    refit_nodes = plain.ReadBVH()[0]
    plain.RebuildBVH(method="ploc")
    assert out["rebuilt"] == 1
    assert same_state(state(auto), state(plain)) and np.array_equal(auto.ReadTriIndices(), plain.ReadTriIndices())
    host = lambda nodes: _cost(nodes)  # noqa: E731
    for key, nodes in (("built", b.nodes), ("refitted", refit_nodes), ("now", plain.ReadBVH()[0])):
        want = host(nodes)
        assert (out[key]["inner_q"], out[key]["leaf_q"], out[key]["n_nodes"]) == (want["inner_q"], want["leaf_q"], want["n_nodes"]), key
    out = kept.Pose(A, rebuild_above=1e9)
    assert out["rebuilt"] == 0 and out["now"] == out["refitted"]
    assert same_bytes(kept.ReadBVH()[0], refit_nodes) and np.array_equal(kept.ReadTriIndices(), b.tri_indices)
    for p in (auto, plain, kept):
        p.destroy()


def _cost(nodes):
    b = api.WideBVH()
    b.nodes = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    return b.Cost()


# ---- 8. several shards on one card ----
def test_two_shards_on_one_device(scene_cache, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = case_of("soup", scene_cache)
    n, nm = len(case.tris), 5
    A = gentle(nm)
    w, h = 64, 36  # 2 x 2 blocks: both shards own some
    for kind in ("parts", "skin"):
        binding = binding_of(kind, n, nm)
        single = tracer(case, case.scene, case.bvh(48), w, h)
        multi = tracer(case, case.scene, case.bvh(48), w, h, cls=api.MultiPathTracer, devices=(0, 0))
        assert multi.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in multi._contexts())
        for t in (single, multi):
            t.Trace(True, 2)
            bind(t, binding, nm)
            t.Pose(A)
            assert t.GetSPP() == 0
            t.Trace(True, SPP)
        a = single.ReadBVH()
        for c in multi._contexts():  # every device posed its own copy
            nodes, woop = np.zeros_like(a[0]), np.zeros_like(a[1])
            N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, woop.ctypes.data), c)
            assert same_bytes(nodes, a[0]) and np.array_equal(bits(woop), bits(a[1]))
        assert multi.GetPoseBinding() == single.GetPoseBinding()
        assert np.array_equal(bits(multi.ReadResult()), bits(single.ReadResult()))
        assert not np.array_equal(bits(single.ReadResult()), np.zeros_like(bits(single.ReadResult())))
        with pytest.raises(N.AdyptError) as e:
            multi.Pose(A[:-1])
        assert e.value.code == N.E_INVALID
        multi.UnbindPose()
        assert multi.GetPoseBinding()["kind"] == 0
        multi.destroy()
        single.destroy()


# ---- 9. timing ----
def test_refit_timing_answers_after_a_pose(scene_cache):
    case = small(257)
    p = tracer(case, case.scene, case.bvh())
    with pytest.raises(N.AdyptError) as e:
        p.GetRefitTiming()
    assert e.value.code == N.E_STATE
    p.BindParts(P.parts_of(257, 3), 3)
    p.Pose(gentle(3))
    ms = p.GetRefitTiming()
    assert set(ms) == {"scatter", "references_woop", "nodes", "total"}
    assert all(np.isfinite(v) and v >= 0.0 for v in ms.values()) and ms["total"] > 0.0
    p.destroy()
