"""What makes the rungs of tests/geometry_edge_inputs.py sharp, held on the CPU, and the host twins held against the numpy truths there.  For every rung:
the branch it exists for is reached — counted on the TRUTH's outputs only (tests/refit_truth.py, pose_truth.py, morph_truth.py, mesh_truth.py,
tree_cost_truth.py, lbvh_truth.py, ploc_truth.py, presplit_truth.py), as inequalities with some room around what they give today — and the host twin
(adypt_bvh_refit, woop_matrices, pose_triangles, mesh_normals, mesh_triangles, adypt_pack_triangles, WideBVH.Cost, BuildLinear, BuildPLOC with and
without a split budget) equals the truth: equal bits, or NaN on both sides at the same words.  The rungs with a NaN among the truth's positions are
derived here and must be exactly geometry_edge_inputs.NAN_POSITIONS.  And the rung at which the host's SBVH builder used not to return: every host
builder refuses it, each in a child process with a time limit.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from adypt_amd import _native as N
from adypt_amd import api
from oracle import oracle_py as O
from tests import geometry_edge_inputs as E
from tests import lbvh_truth as L
from tests import mesh_truth as M
from tests import morph_truth as MO
from tests import ploc_truth as PL
from tests import pose_truth as P
from tests import presplit_truth as S
from tests import refit_truth as T
from tests import tree_cost_truth as TC
from tests import tri_record_truth as R
from tests.probe import same
from tests.test_gpu_pose import small
from tests.test_gpu_refit import same_woop
from tests.test_ploc_definition import lib_tree
from tests.test_presplit_definition import lib_refs
from tests.test_refit_definition import lib_refit, same_bytes
from tests.test_tri_record_definition import lib_pack

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_NORMAL = 2.0 ** -126
CHILD_LIMIT = 60  # seconds


def bands(x):
    """how many of the numbers are 0, denormal, normal, inf, NaN"""
    x = np.asarray(x, dtype=F)
    a = np.abs(x)
    return dict(zero=int((x == 0).sum()), denormal=int(((a > 0) & (a < MIN_NORMAL)).sum()), normal=int(((a >= MIN_NORMAL) & np.isfinite(x)).sum()),
                inf=int(np.isinf(x).sum()), nan=int(np.isnan(x).sum()), all=int(x.size))


def same_triangles(got, want):
    got, want = got.view(O.TRI_DT), want.view(O.TRI_DT)
    return bool(same(got["p"], want["p"]).all() and same(got["n"], want["n"]).all() and got["tc"].tobytes() == want["tc"].tobytes()
                and np.array_equal(got["matid"], want["matid"]))


# ---- coordinates: refit, Woop data, records, cost ----
def coordinate_reach(k, e, woop_nan, cost):
    """e: the exponent bytes of the truth's nodes; woop_nan: NaN words among the 3 084 of the oracle's Woop data; cost: the truth's dict, or None where it refuses"""
    if k == -149:
        return (e == 0).all() and woop_nan == 3084 and cost is None       # cells of 0
    if k in (-140, -126):
        return (e == 1).all() and woop_nan == 3084 and cost is None       # denormal cells: the clamp to 1, the division by 2^-126
    if k == -100:
        return 10 <= e.min() and e.max() <= 40 and woop_nan == 3084 and cost is None  # areas that underflow to 0
    if k in (-64, 40):
        return cost is not None and 500 <= woop_nan <= 2800               # some determinants underflow or overflow, some do not
    if k == 0:
        return cost is not None and woop_nan == 0 and 110 <= e.min() and e.max() <= 130
    if k in (64, 100):
        return cost is None and woop_nan >= 2800 and e.max() < 254        # areas that overflow
    if k == 124:
        return cost is None and e.max() == 254 and e.min() >= 235         # hi - lo near 2^127 and above: the clamp to 254
    raise KeyError(k)


@pytest.mark.parametrize("k", E.COORD_K)
def test_coordinate_rung(k):
    case, tris = small(E.N_TRIS), E.soup(k)
    b = case.bvh()
    assert np.isfinite(tris["p"]).all() and tris["n"].tobytes() == case.tris["n"].tobytes() and (k == 0) == (tris.tobytes() == case.tris.tobytes())
    want = T.refit(b.nodes, b.tri_indices, tris)[0]
    e = want["e"][(want["meta"] != 0).any(axis=1)]
    woop = O.woop_matrices(tris, b.tri_indices)
    try:
        cost = TC.cost(want)
    except ValueError:
        cost = None
    print("k %d: exponent bytes %d .. %d, NaN words in the Woop data %d of %d, cost %s" % (k, e.min(), e.max(), np.isnan(woop).sum(), woop.size, cost))
    assert coordinate_reach(k, e, int(np.isnan(woop).sum()), cost)
    # the twins
    r, got = lib_refit(b.nodes, b.tri_indices, tris)
    assert r == N.ADYPT_OK and same_bytes(got, want), "adypt_bvh_refit"
    assert same_woop(api.woop_matrices(tris, b.tri_indices), woop), "woop_matrices"
    assert lib_pack(tris, case.scene.materials, 0)[0].tobytes() == R.pack(tris, case.scene.materials, 0)[0].tobytes(), "adypt_pack_triangles"
    refitted = api.WideBVH()
    refitted.nodes = got
    if cost is None:
        with pytest.raises(N.AdyptError) as err:
            refitted.Cost()
        assert err.value.code == N.E_INVALID and "no positive finite area" in str(err.value)
    else:
        assert refitted.Cost() == cost, "WideBVH.Cost"


# ---- matrices, weights, morph layers, indices: pose ----
def len2_of(tris, mats, **binding):
    """pose_truth.pose's len2 [n, 3], from its own pieces"""
    Mv = P.vertex_matrices(mats, **binding)
    with np.errstate(all="ignore"):
        C = P.cofactors(Mv)
        nx, ny, nz = (tris["n"][..., a][..., None] for a in range(3))
        q = (((C[..., 0] * nx).astype(F) + (C[..., 1] * ny).astype(F)).astype(F) + (C[..., 2] * nz).astype(F)).astype(F)
        return (((q[..., 0] * q[..., 0]).astype(F) + (q[..., 1] * q[..., 1]).astype(F)).astype(F) + (q[..., 2] * q[..., 2]).astype(F)).astype(F)


def matrix_reach(k, kind, b):
    """b: bands of len2 (771 vertices; under the skin 19 of them have no joint and a len2 of 0)"""
    most = 700 if kind == "parts" else 650
    if k == -75:
        return b["zero"] == b["all"]
    if k == -38:
        return b["zero"] >= most and 5 <= b["denormal"] and b["normal"] == 0       # the first denormal len2 among zeros
    if k in (-37, -36, -33):
        return b["denormal"] >= (600 if kind == "skin" and k == -37 else most) and b["normal"] == 0  # normalised with a denormal len2
    if k in (0, 31):
        return b["normal"] >= most and b["denormal"] == b["inf"] == b["nan"] == 0
    if k == 32:
        return b["normal"] >= 200 and b["inf"] >= 200                                # both sides of the overflow
    if k in (33, 63):
        return b["inf"] >= most and b["normal"] <= 30
    raise KeyError(k)


@pytest.mark.parametrize("k", E.MATRIX_K)
@pytest.mark.parametrize("kind", ["parts", "skin"])
def test_matrix_rung(kind, k):
    tris, mats, binding = small(E.N_TRIS).tris, E.matrices(k), E.binding(kind)
    assert np.isfinite(mats).all() and np.array_equal(mats[:, :, 3], E.matrices(0)[:, :, 3])
    b = bands(len2_of(tris, mats, **binding))
    print("%s k %d: len2 %s" % (kind, k, b))
    assert matrix_reach(k, kind, b)
    want = P.pose(tris, mats, **binding)
    assert np.isfinite(want["p"]).all(), "the positions stay finite on the matrix ladder"
    assert same_triangles(api.pose_triangles(tris, mats, **binding), want), "pose_triangles"


@pytest.mark.parametrize("rung", E.WEIGHT_RUNGS)
def test_weight_rung(rung):
    tris, mats, binding = small(E.N_TRIS).tris, E.matrices(0), E.weight_rung(rung)
    even = binding["weights"][::2]
    Mv = P.vertex_matrices(mats, **binding)[::2, :, :, :3]  # the linear parts of the even triangles' vertex matrices
    want = P.pose(tris, mats, **binding)
    b = bands(Mv)
    print("%s: entries of the vertex matrices %s, NaN positions %d" % (rung, b, np.isnan(want["p"]).sum()))
    if rung == "denormal":
        assert (even == E.TINY).all() and b["denormal"] >= 1000 and b["normal"] == 0   # w * B is a few denormal steps, the sums stay denormal
    elif rung == "min_normal":
        assert (even == E.MIN_NORMAL).all() and b["denormal"] >= 500 and b["normal"] >= 1000  # products on both sides of 2^-126
    else:
        assert (even[..., 1] == F(3e38)).all() and (even[..., [0, 2, 3]] == 1).all() and b["inf"] >= 100 and np.isnan(want["p"]).sum() >= 50
    assert same_triangles(api.pose_triangles(tris, mats, **binding), want), "pose_triangles"


@pytest.mark.parametrize("kind", ["parts", "skin"])
@pytest.mark.parametrize("rung", E.MORPH_RUNGS)
def test_morph_rung(rung, kind):
    tris, mats, binding = small(E.N_TRIS).tris, E.matrices(0), E.binding(kind)
    entries, w = E.morph_rung(rung)
    with np.errstate(all="ignore"):
        products = bands((w[entries[1]][:, None] * entries[2]).astype(F))
        morphed = MO.morph(tris, *entries, w)
        want = MO.pose(tris, mats, entries, w, **binding)
    plain = P.pose(tris, mats, **binding)
    changed = int((morphed["p"].view(np.uint32) != tris["p"].view(np.uint32)).sum() + (morphed["n"].view(np.uint32) != tris["n"].view(np.uint32)).sum())
    print("%s, %s: products %s, words the morph stage changes %d, NaN positions %d" % (rung, kind, products, changed, np.isnan(want["p"]).sum()))
    assert np.isfinite(entries[2]).all() and np.isfinite(w).all()
    if rung == "underflow":
        assert products["normal"] == products["inf"] == 0 and products["denormal"] >= 1000
    elif rung == "large":
        assert products["inf"] == 0 and np.isfinite(want["p"]).all() and float(np.abs(morphed["p"]).max()) >= 2.0 ** 125
    elif rung == "overflow":
        assert products["inf"] >= 500 and np.isnan(morphed["p"]).sum() >= 10 and np.isnan(want["p"]).sum() >= 100
    elif rung == "minus_zero":
        assert (w == 0).all() and np.signbit(w).all() and changed == 0 and same_triangles(want, plain)
    else:
        assert (w == E.TINY).all() and changed >= 300 and not same_triangles(want, plain)  # taken: a layer that is skipped changes nothing
    assert same_triangles(api.pose_triangles(tris, mats, morph=entries, morph_weights=w, **binding), want), "pose_triangles"


def test_index_rungs():
    tris = small(E.N_TRIS).tris
    binding, mats = E.index_rung("skin_top_joint")
    j, w = binding["joints"], binding["weights"]
    for s in range(4):
        live = j[..., s][w[..., s] != 0]
        assert (live == E.TOP).sum() >= 3 and ((live >= 32768) & (live != E.TOP)).sum() >= 3, "slot %d" % s
    assert len(mats) == 65536 and all(not np.array_equal(mats[a], mats[b]) for a, b in ((E.TOP, 32767), (E.TOP, 5), (E.HIGH, E.HIGH - 32768)))
    want = P.pose(tris, mats, **binding)
    assert same_triangles(api.pose_triangles(tris, mats, **binding), want), "pose_triangles, joint 65 535"
    # the pose depends on the two matrices at the top
    for at in (E.TOP, E.HIGH):
        other = np.array(mats)
        other[at] = P.identity()
        assert not same_triangles(P.pose(tris, other, **binding), want)
    binding, mats, entries, w = E.index_rung("morph_top_target")
    assert len(w) == 65536 and w[E.TOP] != 0 and w[E.HIGH] != 0 and (entries[1] == E.TOP).sum() >= 50
    want = MO.pose(tris, mats, entries, w, **binding)
    assert same_triangles(api.pose_triangles(tris, mats, morph=entries, morph_weights=w, **binding), want), "pose_triangles, target 65 535"
    for at in (E.TOP, E.HIGH):
        other = w.copy()
        other[at] = 0
        assert not same_triangles(MO.pose(tris, mats, entries, other, **binding), want)


def test_the_rungs_with_nan_positions_are_the_listed_ones():
    tris = small(E.N_TRIS).tris
    found = []
    for k in E.COORD_K:
        assert not np.isnan(E.soup(k)["p"]).any()
    for name in E.MESHES:
        for k in E.MESH_K:
            assert np.isfinite(E.mesh_positions(name, k)).all()
    with np.errstate(all="ignore"):
        for kind in ("parts", "skin"):
            for k in E.MATRIX_K:
                assert not np.isnan(P.pose(tris, E.matrices(k), **E.binding(kind))["p"]).any()
        for rung in E.WEIGHT_RUNGS:
            if np.isnan(P.pose(tris, E.matrices(0), **E.weight_rung(rung))["p"]).any():
                found.append(("weights", rung, "skin"))
        for rung in E.MORPH_RUNGS:
            for kind in ("parts", "skin"):
                if np.isnan(MO.pose(tris, E.matrices(0), *E.morph_rung(rung), **E.binding(kind))["p"]).any():
                    found.append(("morph", rung, kind))
        binding, mats = E.index_rung("skin_top_joint")
        assert not np.isnan(P.pose(tris, mats, **binding)["p"]).any()
        binding, mats, entries, w = E.index_rung("morph_top_target")
        assert not np.isnan(MO.pose(tris, mats, entries, w, **binding)["p"]).any()
    assert tuple(found) == E.NAN_POSITIONS


# ---- meshes ----
def mesh_reach(name, k, faces, len2, normalised):
    nv, grid = len2["all"], name == "grid"
    if k in (-75, -74):
        return faces["normal"] == 0 and faces["zero"] >= faces["all"] * 3 // 4 and (k == -75 and grid or faces["denormal"] >= 20) and normalised == 0
    if k == -64:
        return faces["denormal"] == faces["all"] and len2["zero"] == nv and normalised == 0
    if k == -38:
        return faces["normal"] == faces["all"] and len2["zero"] >= nv - 2 and normalised <= 2
    if k == -37:
        return len2["denormal"] == normalised and (normalised >= 50 if grid else normalised >= 1)
    if k == -36:
        return len2["denormal"] == normalised and (normalised >= 50 if grid else normalised >= 150)
    if k == -31:
        return normalised == nv and (len2["denormal"] >= 1 if grid else len2["denormal"] >= 250)
    if k == 0:
        return normalised == nv == len2["normal"]
    if k == 31:
        return normalised >= nv - 2 and len2["normal"] >= nv - 2
    if k == 32:
        return len2["inf"] >= 1 and normalised >= 20 and (not grid or len2["inf"] >= 20)
    if k == 33:
        return len2["inf"] >= 50 and (normalised == 0 if grid else normalised >= 150)
    if k == 64:
        return normalised == 0 and len2["inf"] + len2["nan"] == nv
    if k == 100:
        return normalised == 0 and faces["inf"] + faces["nan"] >= faces["all"] * 9 // 10 and len2["nan"] >= 50
    raise KeyError(k)


@pytest.mark.parametrize("k", E.MESH_K)
@pytest.mark.parametrize("name", sorted(E.MESHES))
def test_mesh_rung(name, k):
    idx, pos = E.mesh(name)[0], E.mesh_positions(name, k)
    rest = M.rest_triangles(*E.mesh(name))
    acc = M.sums(idx, pos)[0]
    want, ok = M.normalise(acc)
    with np.errstate(all="ignore"):
        len2 = (acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2]
    faces, len2 = bands(M.faces(idx, pos)), bands(len2)
    print("%s k %d: face vectors %s, len2 %s, normalised %d, NaN words in the normals %d" % (name, k, faces, len2, ok.sum(), np.isnan(want).sum()))
    assert mesh_reach(name, k, faces, len2, int(ok.sum()))
    assert same(api.mesh_normals(idx, pos), want).all(), "mesh_normals"
    assert same_triangles(api.mesh_triangles(rest, idx, pos), M.triangles(rest, idx, pos)), "mesh_triangles"
    for nk in E.GIVEN_NORMAL_K:
        given = E.given_normals(name, nk)
        assert np.isfinite(given).all() and bands(given)["denormal" if nk < 0 else "normal"] >= given.size - 5 and (float(np.abs(given).max()) >= 2.0 ** 120) == (nk > 0)
        got = api.mesh_triangles(rest, idx, pos, given).view(O.TRI_DT)
        assert same_triangles(got, M.triangles(rest, idx, pos, given)) and got["n"].tobytes() == given[idx].tobytes(), "given normals come back as given"


# ---- the builders ----
def host_build(tris, how):
    b = api.WideBVH()
    s, cfg = api.Scene.FromArrays(tris, T.soup_material()), api.InstanceConfig().bvh_params()
    if how == "linear":
        b.BuildLinear(s, cfg)
    elif how == "sbvh":
        cfg.max_spatial_depth = 0
        b.Build(s, cfg)
    else:
        b.BuildPLOC(s, cfg, 8, 0.3 if how == "split" else 0.0)
    return b


@pytest.mark.parametrize("k", E.REBUILD_K)
def test_builders_on_a_coordinate_rung(k):
    tris = E.soup(k)
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    # the keys: 1024 / (hi - lo) is inf for a denormal extent
    c = L.centroids(tris)
    with np.errstate(all="ignore"):
        scale = F(1024.0) / (c.max(axis=0) - c.min(axis=0)).astype(F)
    keys = np.zeros(len(tris), dtype=np.uint64)
    assert N.lib.adypt_lbvh_keys(t.ctypes.data, len(tris), keys.ctypes.data) == N.ADYPT_OK
    assert np.array_equal(keys, np.sort(L.keys(tris))), "the sorted keys"
    print("k %d: 1024 / extent %s, distinct Morton codes %d" % (k, scale, len(np.unique(keys >> np.uint64(32)))))
    assert np.isinf(scale).all() == (k <= -126) and (k > -126) == (len(np.unique(keys >> np.uint64(32))) >= 200)
    # the PLOC pairing
    r, left, right = lib_tree(tris, 8)
    want_left, want_right, _ = PL.tree(tris, 8)
    assert r == N.ADYPT_OK and np.array_equal(left, want_left) and np.array_equal(right, want_right), "adypt_ploc_tree"
    # the references of the pre-split
    level, ref_tri, ref_box = lib_refs(tris, 0.3)
    want_level, want_tri, want_box = S.refs(tris, 0.3)
    assert level == want_level and np.array_equal(ref_tri, want_tri) and same(ref_box, want_box).all(), "adypt_presplit_refs"
    # the trees: valid, and their boxes the truth's refit of their own topology
    for how in ("linear", "ploc", "split"):
        b = host_build(tris, how)
        if how == "split" and len(b.tri_indices) > len(tris):
            continue  # (boxes of clipped references: tests/test_presplit_definition.py)
        L.check_tree(b.nodes, b.tri_indices, len(tris))
        assert same_bytes(T.refit(b.nodes, b.tri_indices, tris)[0], b.nodes), how
        try:
            want = TC.cost(b.nodes)
        except ValueError:
            want = None
        print("k %d %s: %d nodes, cost %s" % (k, how, len(b.nodes) // 80, want))
        assert (want is None) == (k <= -100), "areas that underflow to 0 have no cost"
        if want is None:
            with pytest.raises(N.AdyptError) as err:
                b.Cost()
            assert err.value.code == N.E_INVALID
        else:
            assert b.Cost() == want


CHILD = """
import sys
sys.path.insert(0, %r)
from adypt_amd import _native as N
from tests import geometry_edge_inputs as E
from tests.test_geometry_edge_inputs import host_build
try:
    host_build(E.soup(E.REFUSED_K), sys.argv[1])
    print("built")
except N.AdyptError as e:
    print("refused", e.code == N.E_INVALID, e)
"""


@pytest.mark.parametrize("how", ["linear", "ploc", "split", "sbvh"])
def test_costs_that_overflow_are_refused_by_every_host_builder(how):
    """Node areas of about 2^129 at k = 60: every SAH cost is inf.  The SBVH builder's sweep then named no split (left_n 0) and made the node its own right
    child, without end; the collapse behind the linear builder took such a tree.  Both refuse now, as the device builder does.  In a child process, so
    that a builder that does not return fails this test by its time limit and nothing else."""
    tris = E.soup(E.REFUSED_K)
    lo, hi = tris["p"].reshape(-1, 3).min(axis=0).astype(np.float64), tris["p"].reshape(-1, 3).max(axis=0).astype(np.float64)
    ext = hi - lo
    assert np.isfinite(tris["p"]).all() and 2 * (ext[0] * (ext[1] + ext[2]) + ext[1] * ext[2]) > 2.0 ** 128, "the scene's area is past FLT_MAX"
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, how], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_LIMIT, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    words = out.stdout.decode().split(None, 2)
    print(how, words)
    assert words[:2] == ["refused", "True"]
    assert "infinite or NaN" in words[2] or "not finite numbers below FLT_MAX" in words[2]


def test_rays_hit_at_k_0():
    """the oracle alone: of the 2 048 rays of the k = 0 rung at least a quarter hit, closest hit and any hit alike"""
    case, tris = small(E.N_TRIS), E.soup(0)
    b = case.bvh()
    osc = O.Scene(b.nodes, b.tri_indices, tris, case.scene.materials, woop=api.woop_matrices(tris, b.tri_indices))
    for any_hit in (False, True):
        hits = int((O.trace(osc, E.rays(0), stack_size=32, any_hit=any_hit)["tri_id"] >= 0).sum())
        print("any_hit %s: %d of %d rays hit" % (any_hit, hits, E.N_RAYS))
        assert hits >= E.N_RAYS // 4
