"""-m gpu: the geometry kernels at the numeric edges of finite, accepted input (refit.hip, pose.hip, mesh.hip, build.hip, geometry.hip, the traversal).  The
inputs are tests/geometry_edge_inputs.py's rungs — coordinates, matrices, weights and deltas times 2^k, under which the arithmetic inside the kernels
underflows to denormals and to 0 or overflows to inf and NaN, and joint and target indices at the top of 16 bits; which branch a rung reaches, and that the
host twins equal the numpy truths there, is held on the CPU in tests/test_geometry_edge_inputs.py.  Here the device is held against the host twin compiled
from the same header: equal bits, or NaN on both sides at the same words (a generated NaN is 0xffc00000 on x86 and 0x7fc00000 on gfx950), no tolerance.  That
only holds if the device keeps denormals and its sqrtf and / are the correctly rounded ones down to denormal operands: which of these tests fail with
denormals flushed, and which with the approximate division and square root, is recorded in DESIGN.md ("Held at the numeric edges of finite input").
One test per (operation, rung): a failure names the narrowest thing.  Every scene has at most 302 triangles, the image is 32 x 18, and a context is created
with the host's tree of the rung-0 scene."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import geometry_edge_inputs as E  # noqa: E402
from tests import mesh_truth as M  # noqa: E402
from tests import refit_truth as T  # noqa: E402
from tests import tri_record_truth as R  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.probe import same  # noqa: E402
from tests.test_gpu_mesh import MeshCase  # noqa: E402
from tests.test_gpu_mesh import host_posed as mesh_posed  # noqa: E402
from tests.test_gpu_morph import host_posed  # noqa: E402
from tests.test_gpu_pose import bind, expect_tree, small, state  # noqa: E402
from tests.test_gpu_rebuild import holds  # noqa: E402
from tests.test_gpu_rebuild_split import holds_split  # noqa: E402
from tests.test_gpu_refit import PT, same_woop, tracer  # noqa: E402
from tests.test_gpu_set_triangles import same_info  # noqa: E402
from tests.test_refit_definition import lib_refit, same_bytes  # noqa: E402

BUILD = {"linear": dict(method="linear"), "ploc": dict(method="ploc", radius=8), "split": dict(method="ploc", radius=8, split_budget=0.3)}
_meshes = {}


def fresh():
    """(the rung-0 case, its host tree, a context created with both)"""
    case = small(E.N_TRIS)
    return case, case.bvh(), tracer(case, case.scene, case.bvh())


def same_records(got, want):
    """words 0..17 (positions and normals) in bits or NaN on both sides, the other words in bits"""
    got, want = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 32), np.ascontiguousarray(want).view(np.uint32).reshape(-1, 32)
    return got.shape == want.shape and bool(same(got[:, :18].view(np.float32), want[:, :18].view(np.float32)).all()) and np.array_equal(got[:, 18:], want[:, 18:])


def records_of(case, tris):
    return R.pack(tris, case.scene.materials, 0)[0]


def host_cost(nodes):
    """WideBVH.Cost() of the nodes, or None where it refuses"""
    b = api.WideBVH()
    b.nodes = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    try:
        return b.Cost()
    except N.AdyptError as e:
        assert e.code == N.E_INVALID
        return None


def expect_refit(p, case, b, tris, what):
    """nodes, Woop data, records, reference order and cost after UpdateTriangles to `tris`; returns the host's nodes and Woop data"""
    r, want = lib_refit(b.nodes, b.tri_indices, tris)
    assert r == N.ADYPT_OK
    woop = api.woop_matrices(tris, b.tri_indices)
    nodes, got_woop = p.ReadBVH()
    assert same_bytes(nodes, want), what + ": nodes"
    assert same_woop(got_woop, woop), what + ": Woop data"
    assert same_records(p.ReadTriangleRecords(), records_of(case, tris)), what + ": records"
    assert np.array_equal(p.ReadTriIndices(), b.tri_indices), what + ": the reference order stays"
    cost = host_cost(want)
    if cost is None:
        with pytest.raises(N.AdyptError) as e:
            p.GetTreeCost()
        assert e.value.code == N.E_INVALID, what + ": the cost is refused as on the host"
    else:
        assert p.GetTreeCost() == cost, what + ": the cost"
    return want, woop


# ---- a. refit ----
@pytest.mark.parametrize("k", E.COORD_K)
def test_refit(k):
    case, b, p = fresh()
    for rung in (k, 0):  # ... and back: the context is usable after a rung whose cost is refused
        tris = E.soup(rung)
        p.UpdateTriangles(0, tris["p"].reshape(-1, 9))
        expect_refit(p, case, b, tris, "k %d" % rung)
    p.destroy()


# ---- b. rays after a refit ----
@pytest.mark.parametrize("k", E.RAY_K)
def test_rays(k):
    case, b, p = fresh()
    tris, rays = E.soup(k), E.rays(k)
    p.UpdateTriangles(0, tris["p"].reshape(-1, 9))
    nodes, woop = expect_refit(p, case, b, tris, "k %d" % k)
    osc = O.Scene(nodes, b.tri_indices, tris, case.scene.materials, woop=woop)
    for any_hit in (False, True):
        got, want = p.TraceRays(rays, with_stats=True, any_hit=any_hit), O.trace(osc, rays, stack_size=PT["stack_size"], any_hit=any_hit)
        hits = int((want["tri_id"] >= 0).sum())
        print("k %d any_hit %s: the oracle hits on %d of %d rays" % (k, any_hit, hits, len(rays)))
        for f in api.HIT_DT.names:
            assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), "%s (any_hit %s)" % (f, any_hit)
        assert k != 0 or hits >= len(rays) // 4
    p.destroy()


# ---- c. pose: matrices, weights, morph layers, indices ----
def expect_pose(p, case, b, posed, what, nan_positions=False):
    assert same_records(p.ReadTriangleRecords(), records_of(case, posed)), what + ": records"
    if not nan_positions:  # (with a NaN among the positions the unions depend on their order: geometry_edge_inputs.NAN_POSITIONS)
        expect_tree(p, b, posed, what)


@pytest.mark.parametrize("k", E.MATRIX_K)
@pytest.mark.parametrize("kind", ["parts", "skin"])
def test_pose_matrices(kind, k):
    case, b, p = fresh()
    binding, mats = E.binding(kind), E.matrices(k)
    bind(p, binding, E.N_MATRICES)
    assert p.Pose(mats) is None
    expect_pose(p, case, b, host_posed(case.tris, mats, **binding), "%s, k %d" % (kind, k))
    p.destroy()


@pytest.mark.parametrize("rung", E.WEIGHT_RUNGS)
def test_pose_weights(rung):
    case, b, p = fresh()
    binding, mats = E.weight_rung(rung), E.matrices(0)
    bind(p, binding, E.N_MATRICES)
    p.Pose(mats)
    expect_pose(p, case, b, host_posed(case.tris, mats, **binding), rung, ("weights", rung, "skin") in E.NAN_POSITIONS)
    p.destroy()


@pytest.mark.parametrize("kind", ["parts", "skin"])
@pytest.mark.parametrize("rung", E.MORPH_RUNGS)
def test_pose_morph(rung, kind):
    case, b, p = fresh()
    binding, mats = E.binding(kind), E.matrices(0)
    entries, w = E.morph_rung(rung)
    bind(p, binding, E.N_MATRICES)
    p.BindMorph(*entries, E.N_TARGETS)
    p.Pose(mats, morph_weights=w)
    expect_pose(p, case, b, host_posed(case.tris, mats, entries, w, **binding), "%s, %s" % (rung, kind), ("morph", rung, kind) in E.NAN_POSITIONS)
    if rung == "minus_zero":  # skipped like a weight of +0: the bytes of a pose without weights, which leaves the rest pose's bits to the matrices
        got = state(p)
        p.Pose(mats)
        plain = state(p)
        assert got[0].tobytes() == plain[0].tobytes() and same_bytes(got[1], plain[1]) and np.array_equal(bits(got[2]), bits(plain[2]))
    p.destroy()


def test_pose_top_joint():
    case, b, p = fresh()
    binding, mats = E.index_rung("skin_top_joint")
    p.BindSkin(binding["joints"], binding["weights"], len(mats))
    assert p.GetPoseBinding()["n_matrices"] == 65536
    p.Pose(mats)
    expect_pose(p, case, b, host_posed(case.tris, mats, **binding), "joints 65 535 and 40 000")
    p.destroy()


def test_pose_top_target():
    case, b, p = fresh()
    binding, mats, entries, w = E.index_rung("morph_top_target")
    bind(p, binding, E.N_MATRICES)
    p.BindMorph(*entries, len(w))
    assert p.GetMorphBinding()["n_targets"] == 65536
    p.Pose(mats, morph_weights=w)
    expect_pose(p, case, b, host_posed(case.tris, mats, entries, w, **binding), "targets 65 535 and 40 000")
    p.destroy()


# ---- d. meshes ----
def mesh_case(name):
    if name not in _meshes:
        _meshes[name] = MeshCase(*E.mesh(name))
    return _meshes[name]


@pytest.mark.parametrize("k", E.MESH_K)
@pytest.mark.parametrize("name", sorted(E.MESHES))
def test_mesh(name, k):
    case = mesh_case(name)
    idx, nv, pos = case.idx, len(case.p), E.mesh_positions(name, k)
    b = case.bvh()
    p = tracer(case, case.scene, b)
    p.BindMesh(idx, nv)
    ref = M.referenced(idx, nv)
    assert p.PoseVertices(pos) is None
    assert same(p.ReadVertexNormals()[ref], api.mesh_normals(idx, pos)[ref]).all(), "the vertex normals"
    posed = mesh_posed(case.tris, idx, pos)
    assert same_records(p.ReadTriangleRecords(), records_of(case, posed)), "records"
    expect_tree(p, b, posed, "%s, k %d" % (name, k))
    for nk in E.GIVEN_NORMAL_K:  # used as given: back to the bit
        given = E.given_normals(name, nk)
        p.PoseVertices(pos, given)
        assert np.array_equal(bits(p.ReadVertexNormals())[ref], bits(given)[ref]), "given normals times 2^%d" % nk
        assert p.ReadTriangleRecords().tobytes() == records_of(case, mesh_posed(case.tris, idx, pos, given)).tobytes(), "records with given normals times 2^%d" % nk
    p.destroy()


# ---- e. rebuild ----
def host_build(tris, method):
    b = api.WideBVH()
    s, cfg = api.Scene.FromArrays(tris, T.soup_material()), api.InstanceConfig().bvh_params()
    if method == "linear":
        b.BuildLinear(s, cfg)
    else:
        b.BuildPLOC(s, cfg, 8, 0.3 if method == "split" else 0.0)
    return b, api.woop_matrices(tris, b.tri_indices)


@pytest.mark.parametrize("method", sorted(BUILD))
@pytest.mark.parametrize("k", E.REBUILD_K)
def test_rebuild(k, method):
    case, _, p = fresh()
    tris = E.soup(k)
    p.SetTriangles(tris)
    assert p.GetTriangleCount() == len(tris) and same_records(p.ReadTriangleRecords(), records_of(case, tris))
    b, woop = host_build(tris, method)
    info = p.RebuildBVH(**BUILD[method])
    split = len(b.tri_indices) > len(tris)
    print("k %d %s: %s, %d references" % (k, method, info, len(b.tri_indices)))
    assert (holds_split if split else holds)(p, b, woop), "nodes, reference order, Woop data" + (", reference boxes" if split else "")
    assert split or p.ReadRefBoxes() is None
    assert same_info(info, b) and p.GetBVHSizes() == (len(b.nodes) // 80, len(b.tri_indices))
    p.destroy()


@pytest.mark.parametrize("method", sorted(BUILD))
def test_rebuild_refused(method):
    """k = 60: node areas of about 2^129, every SAH cost of an inner node overflows.  The host's builders refuse (tests/test_geometry_edge_inputs.py), and
    so must the device, with the same code and the context as it was.  That the device ends there was read in build.hip, not tried: linear — k_radix_tree's
    searches double and halve a step over unique keys (lbvh.hpp lbvh_inner_node: lbvh_delta is -1 outside the list, so `while(... > dmin)` ends within
    log2 n steps), k_bottom_up climbs `parent` from a leaf and leaves at the first node it reaches first, cut_forest_wide's stack holds 8 entries and breaks
    beyond, and rebuild() returns at its check of kFlagCost (build.hip:708) before the emission loop.  PLOC — ploc_nearest scans 2 r positions, and every
    trip of ploc_rounds' loop either returns (kFlagCost at 554, kFlagLayout at 555, `merges <= 0 || stay != m - merges` at 556) or goes on with m - merges
    < m clusters: at most n - 1 trips.  With a split budget — presplit_walk goes down at most kSplitMaxDepth levels and every trip either descends or
    emits a leaf, presplit_bin and presplit_level count up to kSplitLevels; then the PLOC path."""
    case, b, p = fresh()
    tris = E.soup(E.REFUSED_K)
    with pytest.raises(N.AdyptError) as e:
        host_build(tris, method)
    assert e.value.code == N.E_INVALID
    p.UpdateTriangles(0, tris["p"].reshape(-1, 9))  # (a refit builds nothing)
    before, order = state(p), p.ReadTriIndices()
    assert same_bytes(before[1], lib_refit(b.nodes, b.tri_indices, tris)[1])
    with pytest.raises(N.AdyptError) as e:
        p.RebuildBVH(**BUILD[method])
    assert e.value.code == N.E_INVALID, str(e.value)
    after = state(p)
    assert after[0].tobytes() == before[0].tobytes() and same_bytes(after[1], before[1]) and np.array_equal(bits(after[2]), bits(before[2]))
    assert np.array_equal(p.ReadTriIndices(), order) and p.GetBVHSizes() == (len(b.nodes) // 80, len(b.tri_indices))
    # ... and usable: back at rung 0 it rebuilds
    rest = E.soup(0)
    p.UpdateTriangles(0, rest["p"].reshape(-1, 9))
    want, woop = host_build(rest, method)
    info = p.RebuildBVH(**BUILD[method])
    assert (holds_split if len(want.tri_indices) > len(rest) else holds)(p, want, woop) and same_info(info, want)
    p.destroy()
