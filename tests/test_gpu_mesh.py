"""-m gpu: an indexed mesh posed by its vertices on the device (include/adypt_hip.h adypt_bind_mesh, adypt_pose_vertices; k_mesh_faces, k_mesh_normals,
k_mesh_records in csrc/device/mesh.hip).  The device's triangle records after PoseVertices() are held against the host's adypt_mesh_triangles packed by
tests/tri_record_truth.py byte for byte (and that function against numpy in tests/test_mesh_definition.py), the vertex normals against
adypt_mesh_normals in bits; records, nodes and Woop data against a second tracer that was given the host-made arrays through UpdateTriangles; the tree
against adypt_bvh_refit + adypt_woop_matrices; images against the CPU oracle, bit for bit.  A workgroup takes 256 triangles or vertices, a wave 64:
fan(k) puts the triangle count k and the vertex count k + 2 on both sides of both, and its apex's list is one lane's loop of k trips beside lanes
with one or two."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import mesh_truth as M  # noqa: E402
from tests import refit_truth as T  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_gpu_pose import expect_tree, records_of, same_state, state  # noqa: E402
from tests.test_gpu_refit import SPP, case_of, oracle_image, tracer  # noqa: E402
from tests.test_refit_definition import same_bytes  # noqa: E402

NONE = {"n_vertices": 0, "n_tris": 0, "max_valence": 0, "device_bytes": 0}
_meshes, _welded = {}, {}


class MeshCase:
    """what tracer() asks of a case, for a mesh of tests/mesh_truth.py: its triangles with computed normals as the rest pose"""

    def __init__(self, indices, positions):
        self.idx, self.p = indices, positions
        self.tris = M.rest_triangles(indices, positions)
        self.tris.setflags(write=False)
        self.scene = api.Scene.FromArrays(self.tris, T.soup_material())
        self.ip, self.iv = api.camera_matrices(60.0, 30.0, -10.0, 32, 18)
        self.pos = np.zeros(3, np.float32)
        self._b = None

    def bvh(self, depth=48):
        if self._b is None:
            cfg = api.InstanceConfig().bvh_params()
            cfg.max_spatial_depth = 0  # (no spatial splits: two coincident triangles would be split without end)
            self._b = api.WideBVH()
            self._b.Build(self.scene, cfg)
            self._b.nodes.setflags(write=False)
        return self._b


MESHES = {"grid": lambda: M.grid(40, 32), "pair": M.opposite_pair, "unreferenced": M.with_unreferenced, "doubled": M.with_doubled_index}
FANS = (1, 63, 64, 65, 253, 254, 255, 256, 257, 300)


def mesh_case(name):
    if name not in _meshes:
        _meshes[name] = MeshCase(*(M.fan(name) if isinstance(name, int) else MESHES[name]()))
    return _meshes[name]


def welded(name, cache):
    """(case, indices, positions, normals) of tiny0 or the soup welded"""
    if name not in _welded:
        case = case_of(name, cache)
        _welded[name] = (case,) + api.weld_triangles(case.tris)
    return _welded[name]


def host_posed(tris, idx, pos, nrm=None):
    t = api.mesh_triangles(tris, idx, pos, nrm).view(O.TRI_DT)
    t.setflags(write=False)
    return t


def update(p, tris):
    p.UpdateTriangles(0, tris["p"].reshape(-1, 9), tris["n"].reshape(-1, 9))


# ---- 1. records and vertex normals ----
@pytest.mark.parametrize("name", FANS + tuple(sorted(MESHES)))
def test_records_equal_the_host_definition(name):
    case = mesh_case(name)
    idx, nv, n = case.idx, len(case.p), len(case.idx)
    p = tracer(case, case.scene, case.bvh())
    rest = p.ReadTriangleRecords()
    assert p.GetMeshBinding() == NONE
    p.BindMesh(idx, nv)
    got = p.GetMeshBinding()
    assert (got["n_vertices"], got["n_tris"], got["max_valence"]) == (nv, n, int(np.bincount(idx.ravel()).max()))
    assert got["device_bytes"] >= 40 * n + 32 * nv + 8  # DESIGN.md, Poses given by vertices: memory
    if isinstance(name, int):
        assert got["max_valence"] == name
    ref = M.referenced(idx, nv)
    for seed in (1, 2):
        pos = M.deform(case.p, seed)
        for given in (None, M.some_normals(nv, seed)):
            assert p.PoseVertices(pos, given) is None
            rec = p.ReadTriangleRecords()
            assert rec.tobytes() == records_of(case, host_posed(case.tris, idx, pos, given)).tobytes(), (seed, given is None)
            assert np.array_equal(rec[:, 18:], rest[:, 18:])  # material id, class word, texture coordinates, zeros: their bytes
            assert not np.array_equal(rec[:, :9], rest[:, :9])
            want = api.mesh_normals(idx, pos) if given is None else given
            assert np.array_equal(bits(p.ReadVertexNormals())[ref], bits(want)[ref]), (seed, given is None)
    p.UnbindMesh()
    assert p.GetMeshBinding() == NONE
    p.destroy()


# ---- 2. the device state is that of an update with the host-made arrays ----
@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("name", ["tiny0", "soup"])
def test_state_equals_an_update_with_host_arrays(name, given, scene_cache):
    case, idx, rest_p, rest_n = welded(name, scene_cache)
    pos = M.deform(rest_p, 3)
    nrm = M.some_normals(len(pos)) if given else None
    posed = host_posed(case.tris, idx, pos, nrm)
    by_vertices, by_update = tracer(case, case.scene, case.bvh(48)), tracer(case, case.scene, case.bvh(48))
    by_vertices.BindMesh(idx)
    by_vertices.PoseVertices(pos, nrm)
    update(by_update, posed)
    assert same_state(state(by_vertices), state(by_update))
    assert by_vertices.GetSPP() == 0
    # the welded rest pose with its own normals is the scene as loaded
    by_vertices.PoseVertices(rest_p, rest_n)
    assert by_vertices.ReadTriangleRecords().tobytes() == records_of(case, case.tris).tobytes()
    by_update.destroy()
    by_vertices.destroy()


# ---- 3. tree and image ----
@pytest.mark.parametrize("name", ["tiny0", "soup"])
def test_tree_and_image_after_a_vertex_pose(name, scene_cache, sobol_matrices):
    case, idx, rest_p, _ = welded(name, scene_cache)
    b = case.bvh(48)
    pos = M.deform(rest_p, 3)
    posed = host_posed(case.tris, idx, pos)
    p = tracer(case, case.scene, b)
    p.Trace(True, 2)  # (the rest pose has been rendered: per-reference records, primary-hit cache and image are its)
    p.BindMesh(idx)
    p.PoseVertices(pos)
    assert p.GetSPP() == 0
    want_nodes = expect_tree(p, b, posed)
    assert not same_bytes(want_nodes, b.nodes)
    if name == "tiny0":
        p.Trace(True, SPP)
        want = oracle_image(case, want_nodes, b.tri_indices, posed, sobol_matrices)
        assert np.array_equal(bits(p.ReadResult()), bits(want)), "the image of the posed mesh"
        assert not np.array_equal(bits(want), bits(oracle_image(case, b.nodes, b.tri_indices, case.tris, sobol_matrices)))  # the pose shows
    p.destroy()


# ---- 4. no compounding ----
def test_vertex_poses_do_not_compound(scene_cache):
    case, idx, rest_p, _ = welded("tiny0", scene_cache)
    A, B = M.deform(rest_p, 1), M.deform(rest_p, 2)
    p = tracer(case, case.scene, case.bvh(48))
    p.BindMesh(idx)
    p.PoseVertices(A)
    first = state(p)
    p.PoseVertices(B, M.some_normals(len(B)))
    assert not same_state(state(p), first)
    p.PoseVertices(A)
    assert same_state(state(p), first)
    assert first[0].tobytes() == records_of(case, host_posed(case.tris, idx, A)).tobytes()
    p.destroy()


# ---- 5. policy ----
def test_vertex_pose_under_a_policy(scene_cache):
    case, idx, rest_p, _ = welded("soup", scene_cache)
    pos = M.deform(rest_p, 3)
    b = case.bvh(48)
    auto, plain, kept = (tracer(case, case.scene, b) for _ in range(3))
    for p in (auto, plain, kept):
        p.BindMesh(idx)
    out = auto.PoseVertices(pos, rebuild_above=0, method="ploc", radius=8)
    plain.PoseVertices(pos)
    refit_nodes = plain.ReadBVH()[0]
    plain.RebuildBVH(None, "ploc", 8)
    assert out["rebuilt"] == 1
    assert same_state(state(auto), state(plain)) and np.array_equal(auto.ReadTriIndices(), plain.ReadTriIndices())
    out = kept.PoseVertices(pos, rebuild_above=1e9)
    assert out["rebuilt"] == 0 and out["now"] == out["refitted"]
    assert same_bytes(kept.ReadBVH()[0], refit_nodes) and np.array_equal(kept.ReadTriIndices(), b.tri_indices)
    assert kept.ReadTriangleRecords().tobytes() == records_of(case, host_posed(case.tris, idx, pos)).tobytes()
    for p in (auto, plain, kept):
        p.destroy()


# ---- 6. lifetime ----
def test_binding_lifetime(scene_cache):
    case, idx, rest_p, _ = welded("soup", scene_cache)
    A, B = M.deform(rest_p, 1), M.deform(rest_p, 2)
    p = tracer(case, case.scene, case.bvh(48))
    with pytest.raises(N.AdyptError) as e:
        p.PoseVertices(A)
    assert e.value.code == N.E_STATE
    p.BindMesh(idx)
    bound = p.GetMeshBinding()
    with pytest.raises(N.AdyptError) as e:
        p.ReadVertexNormals()  # (no pose since the bind)
    assert e.value.code == N.E_STATE
    # a rebuild keeps the binding: the pose refits the rebuilt tree
    p.RebuildBVH(method="ploc")
    built = api.WideBVH()
    built.nodes, built.tri_indices = p.ReadBVH()[0], p.ReadTriIndices()
    assert p.GetMeshBinding() == bound
    p.PoseVertices(A)
    expect_tree(p, built, host_posed(case.tris, idx, A), "after a rebuild")
    # independent of the pose binding; the last writer of the records stands, and a BindParts captures what a vertex pose left
    p.BindParts(np.zeros(len(case.tris), np.int32), 1)
    assert p.GetMeshBinding() == bound and p.GetPoseBinding()["kind"] == 1
    p.PoseVertices(B)
    p.Pose(np.eye(3, 4, dtype=np.float32)[None])
    assert p.GetMeshBinding() == bound
    p.PoseVertices(B)
    assert p.ReadTriangleRecords().tobytes() == records_of(case, host_posed(case.tris, idx, B)).tobytes()
    p.UpdateTriangles(0, case.tris["p"].reshape(-1, 9), case.tris["n"].reshape(-1, 9))
    assert p.ReadTriangleRecords().tobytes() == records_of(case, case.tris).tobytes() and p.GetMeshBinding() == bound
    # UnbindMesh
    p.UnbindMesh()
    assert p.GetMeshBinding() == NONE and p.GetPoseBinding()["kind"] == 1
    with pytest.raises(N.AdyptError) as e:
        p.PoseVertices(A)
    assert e.value.code == N.E_STATE
    # new triangles drop the binding
    p.BindMesh(idx)
    p.SetTriangles(case.scene.triangles)
    assert p.GetMeshBinding() == NONE
    with pytest.raises(N.AdyptError) as e:
        p.PoseVertices(A)
    assert e.value.code == N.E_STATE
    p.destroy()


# ---- 7. refusals ----
def test_refusals_change_nothing(scene_cache):
    case, idx, rest_p, _ = welded("tiny0", scene_cache)
    n, nv = len(idx), len(rest_p)
    A = M.deform(rest_p, 1)
    nrm = M.some_normals(nv)
    p = tracer(case, case.scene, case.bvh(48))
    c = p._ctx
    p.BindMesh(idx)
    p.PoseVertices(A)
    before, bound, normals = state(p), p.GetMeshBinding(), p.ReadVertexNormals()
    p.Trace(True, SPP)
    image = p.ReadResult()

    def bad(a, at, value):
        a = a.copy()
        a[at] = value
        return a

    refusals = [
        ("indices is null", lambda: N.lib.adypt_bind_mesh(c, None, n, nv)),
        ("positions is null", lambda: N.lib.adypt_pose_vertices(c, None, None, nv, None, None, None)),
        ("fewer triangles", lambda: p.BindMesh(idx[:-1], nv)),
        ("more triangles", lambda: p.BindMesh(np.concatenate([idx, idx[:1]]), nv)),
        ("no vertices", lambda: N.lib.adypt_bind_mesh(c, idx.ctypes.data, n, 0)),
        ("too many vertices", lambda: N.lib.adypt_bind_mesh(c, idx.ctypes.data, n, 2 ** 31)),
        ("an index below 0", lambda: p.BindMesh(bad(idx, (n // 2, 1), -1), nv)),
        ("an index past the last", lambda: p.BindMesh(bad(idx, (n - 1, 2), nv), nv)),
        ("fewer vertices than the indices name", lambda: p.BindMesh(idx, nv - 1)),
        ("fewer positions", lambda: p.PoseVertices(A[:-1])),
        ("more positions", lambda: p.PoseVertices(np.concatenate([A, A[:1]]))),
        ("a NaN position", lambda: p.PoseVertices(bad(A, (nv // 2, 0), np.nan))),
        ("an infinite position", lambda: p.PoseVertices(bad(A, (nv - 1, 2), np.inf))),
        ("a NaN given normal", lambda: p.PoseVertices(A, bad(nrm, (0, 1), np.nan))),
        ("an infinite given normal", lambda: p.PoseVertices(A, bad(nrm, (nv - 1, 2), -np.inf))),
        ("a negative threshold", lambda: p.PoseVertices(A, rebuild_above=-1.0)),
        ("a radius out of range", lambda: p.PoseVertices(A, rebuild_above=0.0, radius=0)),
    ]
    for what, call in refusals:
        try:
            code = call()
        except N.AdyptError as err:
            code = err.code
        assert code == N.E_INVALID, what
        assert same_state(state(p), before), what
        assert p.GetSPP() == SPP and np.array_equal(bits(p.ReadResult()), bits(image)), what  # not even the accumulation
        assert p.GetMeshBinding() == bound and np.array_equal(bits(p.ReadVertexNormals()), bits(normals)), what
    # the refused binds have left the binding in place: the next pose is its
    B = M.deform(rest_p, 2)
    p.PoseVertices(B, nrm)
    assert p.ReadTriangleRecords().tobytes() == records_of(case, host_posed(case.tris, idx, B, nrm)).tobytes()
    p.destroy()


# ---- 8. several shards on one card ----
def test_two_shards_on_one_device(scene_cache, sobol_matrices, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case, idx, rest_p, _ = welded("tiny0", scene_cache)
    pos = M.deform(rest_p, 3)
    wd, h = 64, 36  # 2 x 2 blocks: both shards own some
    single = tracer(case, case.scene, case.bvh(48), wd, h)
    multi = tracer(case, case.scene, case.bvh(48), wd, h, cls=api.MultiPathTracer, devices=(0, 0))
    assert multi.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in multi._contexts())
    for t in (single, multi):
        t.Trace(True, 2)
        t.BindMesh(idx)
        t.PoseVertices(pos)
        assert t.GetSPP() == 0
        t.Trace(True, SPP)
    want = state(single)
    for c in multi._contexts():  # every device posed its own copy
        nodes, woop = np.zeros_like(want[1]), np.zeros_like(want[2])
        N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, woop.ctypes.data), c)
        assert same_bytes(nodes, want[1]) and np.array_equal(bits(woop), bits(want[2]))
    assert multi.ReadTriangleRecords().tobytes() == want[0].tobytes()
    assert multi.GetMeshBinding() == single.GetMeshBinding() and multi.GetMeshBinding()["n_vertices"] == len(pos)
    assert np.array_equal(bits(multi.ReadVertexNormals()), bits(single.ReadVertexNormals()))
    assert np.array_equal(bits(multi.ReadResult()), bits(single.ReadResult()))
    assert not np.array_equal(bits(single.ReadResult()), np.zeros_like(bits(single.ReadResult())))
    for call in (lambda: multi.PoseVertices(pos[:-1]), lambda: multi.BindMesh(idx + 1, len(pos))):
        with pytest.raises(N.AdyptError) as e:
            call()
        assert e.value.code == N.E_INVALID
    assert multi.GetMeshBinding() == single.GetMeshBinding()
    multi.UnbindMesh()
    assert multi.GetMeshBinding() == NONE
    multi.destroy()
    single.destroy()


# ---- 9. timing ----
def test_refit_timing_answers_after_a_vertex_pose():
    case = mesh_case(257)
    p = tracer(case, case.scene, case.bvh())
    p.BindMesh(case.idx, len(case.p))
    with pytest.raises(N.AdyptError) as e:
        p.GetMeshTiming()
    assert e.value.code == N.E_STATE
    pos = M.deform(case.p, 1)
    p.PoseVertices(pos)
    ms, stages = p.GetRefitTiming(), p.GetMeshTiming()
    assert set(ms) == {"scatter", "references_woop", "nodes", "total"}
    assert all(np.isfinite(v) and v >= 0.0 for v in ms.values()) and ms["total"] > 0.0 and ms["scatter"] > 0.0
    # the stages of the mesh kernels lie inside the refit's first
    assert set(stages) == {"upload", "faces", "normals", "records"} and all(np.isfinite(v) and v > 0.0 for v in stages.values())
    assert sum(stages.values()) <= ms["scatter"] + 0.01
    p.PoseVertices(pos, M.some_normals(len(pos)))
    stages = p.GetMeshTiming()
    assert stages["records"] > 0.0 and stages["upload"] > 0.0 and stages["faces"] == 0.0 and stages["normals"] == 0.0  # (given normals: those kernels do not run)
    assert sum(stages.values()) <= p.GetRefitTiming()["scatter"] + 0.01
    p.PoseVertices(pos)  # (and computed again, behind a pose with given normals)
    assert all(v > 0.0 for v in p.GetMeshTiming().values())
    p.destroy()
