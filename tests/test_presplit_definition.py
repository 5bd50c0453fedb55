"""Splitting large triangles before the PLOC build, on the host: adypt_presplit_refs and adypt_bvh_build_ploc_split (csrc/device/presplit.hpp) against the
numpy restatement (tests/presplit_truth.py), against a binary64 clip of the same cells, against the refit, against the SBVH builder's tree through the
CPU oracle, and against the unsplit PLOC tree in what the splits are for: less leaf area, fewer triangle tests and nodes per ray — on a mesh with
long thin triangles across it; no claim is made on triangles of similar size.  No GPU."""
import functools

import numpy as np
import pytest

from adypt_amd import _native as N
from adypt_amd import api
from oracle import oracle_py as O
from tests import lbvh_truth as L
from tests import presplit_truth as S
from tests import refit_truth as T
from tests.helpers import bits
from tests.test_ploc_definition import DEGENERATE, build_ploc, height_field
from tests.test_refit_definition import build, lib_refit, rest, same_bytes

BUDGETS = (0.1, 0.3, 1.0)


@functools.lru_cache(maxsize=None)
def beams(m, k):
    """height_field(m) without its two wall triangles, and k beams of two long thin triangles each across the volume"""
    field = height_field(m)[:-2]
    quads = []
    for i in range(k):
        a = np.array([-10.0, -2 + 8 * ((7 * i) % k) / k, -10 + 20 * ((5 * i + 3) % k) / k])
        b = np.array([10.0, -2 + 8 * ((11 * i + 5) % k) / k, -10 + 20 * ((3 * i + 1) % k) / k])
        if i % 2:
            a, b = a[[2, 1, 0]], b[[2, 1, 0]]
        up = np.array([0.0, 0.3, 0.0])
        quads += [[a, b, b + up], [a, b + up, a + up]]
    t = T.soup(len(field) + 2 * k, 5)
    t["p"] = np.concatenate([field["p"], np.array(quads, np.float32)])
    return t


@functools.lru_cache(maxsize=None)
def triangles(name):
    if name == "soup5000":
        return T.soup(5000)
    if name.startswith("beams"):
        return beams(*(int(x) for x in name[5:].split("x")))
    if name in DEGENERATE:
        return DEGENERATE[name]()
    return rest(name)[0]


def materials(name):
    return rest(name)[1] if name.startswith("tiny") else T.soup_material()


@functools.lru_cache(maxsize=None)
def histogram(name):
    return S.histogram(S.positions(triangles(name)))


def lib_refs(tris, budget):
    """adypt_presplit_refs: (level, ref_tri, ref_box [r, 6])"""
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    level = N.C.c_int32(-9)
    n = N.lib.adypt_presplit_refs(t.ctypes.data, len(tris), budget, 0, N.C.byref(level), None, None)
    assert n >= len(tris), n
    tri, box = np.full(n, -7, np.int32), np.zeros((n, 6), np.float32)
    assert N.lib.adypt_presplit_refs(t.ctypes.data, len(tris), budget, n, N.C.byref(level), tri.ctypes.data, box.ctypes.data) == n
    return level.value, tri, box


def build_split(tris, mats, budget, threads=None):
    sc = api.Scene.FromArrays(tris, mats)
    b = api.WideBVH()
    if threads is not None:
        N.lib.adypt_host_set_threads(threads)
    try:
        b.BuildPLOC(sc, api.InstanceConfig().bvh_params(), 8, budget)
    finally:
        if threads is not None:
            N.lib.adypt_host_set_threads(0)
    return sc, b


def test_the_fixture():
    assert len(beams(8, 4)) == 136 and len(beams(24, 8)) == 1168 and len(beams(48, 24)) == 4656


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", ["tiny0", "tiny1", "soup5000", "beams24x8"])
def test_library_equals_numpy(name, budget):
    tris = triangles(name)
    level, tri, box = lib_refs(tris, budget)
    want_level, want_tri, want_box = S.refs(tris, budget, histogram(name))
    print("%s budget %.1f: level %d, %d references of %d triangles" % (name, budget, level, len(tri), len(tris)))
    assert level == want_level and np.array_equal(tri, want_tri) and np.array_equal(bits(box), bits(want_box))


@pytest.mark.parametrize("budget", [0.3, 1.0])
@pytest.mark.parametrize("what", sorted(DEGENERATE))
def test_degenerate_inputs(what, budget):
    tris = triangles(what)
    level, tri, box = lib_refs(tris, budget)
    want_level, want_tri, want_box = S.refs(tris, budget)
    assert level == want_level and np.array_equal(tri, want_tri) and np.array_equal(bits(box), bits(want_box))
    per_triangle = np.bincount(tri, minlength=len(tris))
    assert (per_triangle >= 1).all()
    if what == "copies":
        assert len(set(per_triangle)) == 1  # all split alike, or none
    if what == "one":
        assert len(tri) == 1 + (budget == 1.0 and level >= 1)  # (the one triangle is its own scene box: area == S, so it splits from level 1 on)
    _, b = build_split(tris, T.soup_material(), budget)
    assert np.array_equal(np.sort(b.tri_indices), np.sort(tri))


def clip64(p, lo, hi):
    """the triangles p [N, 3, 3] clipped against the boxes [lo, hi] in binary64, no pad: (vertices [N, 9, 3], their number [N])"""
    poly, cnt = np.zeros((len(p), S.POLYGON, 3)), np.full(len(p), 3, np.int64)
    poly[:, :3] = p
    for k in range(3):
        kk = np.full(len(p), k)
        poly, cnt = S.clip_plane(poly, cnt, kk, lo[:, k].astype(np.float64), True)
        poly, cnt = S.clip_plane(poly, cnt, kk, hi[:, k].astype(np.float64), False)
    return poly, cnt


def random_triangles(n, seed=21):
    rs = np.random.RandomState(seed)
    t = T.soup(n, seed)
    scale = 10.0 ** rs.uniform(-1, 3, size=(n, 1, 1))
    t["p"] = (rs.uniform(-1, 1, size=(n, 1, 3)) * scale + rs.normal(0, 0.3, size=(n, 3, 3)) * scale).clip(-1e3, 1e3).astype(np.float32)
    return t


@pytest.mark.parametrize("name", ["random2000", "beams24x8"])
def test_containment(name):
    """Every reference's box contains, with zero allowance, what a binary64 clip of the triangle against the reference's cell leaves; the boxes of a
    triangle together contain its vertices.  Printed: by how much the unpadded binary32 clip falls short, in units of 2^-24 max |v_k| — the pad is 16."""
    tris = random_triangles(2000) if name == "random2000" else triangles(name)
    p = S.positions(tris)
    level, tri, box = lib_refs(tris, 1.0)
    s = S.scene_area(p)
    _, (t_tri, t_lo, t_hi, cell_lo, cell_hi) = S.walk(p, S.threshold(s, level))
    assert np.array_equal(tri, t_tri) and np.array_equal(bits(box), bits(np.concatenate([t_lo, t_hi], axis=1)))
    assert len(tri) > len(tris) + len(tris) // 4
    poly, cnt = clip64(p[tri].astype(np.float64), cell_lo, cell_hi)
    assert (cnt > 0).all()
    valid = np.arange(S.POLYGON)[None, :, None] < cnt[:, None, None]
    lo64, hi64 = np.where(valid, poly, np.inf).min(axis=1), np.where(valid, poly, -np.inf).max(axis=1)
    assert (box[:, :3].astype(np.float64) <= lo64).all() and (box[:, 3:].astype(np.float64) >= hi64).all()
    # the union of a triangle's boxes holds its three vertices
    ulo, uhi = np.full((len(tris), 3), np.inf), np.full((len(tris), 3), -np.inf)
    np.minimum.at(ulo, tri, box[:, :3])
    np.maximum.at(uhi, tri, box[:, 3:])
    assert (ulo <= p.min(axis=1)).all() and (uhi >= p.max(axis=1)).all()
    # the measurement: the same walk without the pad, against the binary64 clip of ITS cells
    _, (m_tri, m_lo, m_hi, mc_lo, mc_hi) = S.walk(p, S.threshold(s, level), pad_scale=0.0)
    poly, cnt = clip64(p[m_tri].astype(np.float64), mc_lo, mc_hi)
    valid = np.arange(S.POLYGON)[None, :, None] < cnt[:, None, None]
    lo64, hi64 = np.where(valid, poly, np.inf).min(axis=1), np.where(valid, poly, -np.inf).max(axis=1)
    unit = np.abs(p[m_tri]).max(axis=1).astype(np.float64) * 2.0 ** -24
    short = np.maximum(m_lo - lo64, hi64 - m_hi)[cnt > 0] / np.maximum(unit[cnt > 0], 1e-300)
    print("%s: %d references; the unpadded binary32 box is short by at most %.2f x 2^-24 max|v_k|" % (name, len(tri), max(short.max(), 0.0)))
    assert short.max() < 16.0  # (else the pad of 2^-20 would be short: enlarge it)


@pytest.mark.parametrize("budget", BUDGETS)
@pytest.mark.parametrize("name", ["tiny0", "soup5000", "beams24x8"])
def test_budget(name, budget):
    tris = triangles(name)
    level, tri, _ = lib_refs(tris, budget)
    allowed = int(np.floor(budget * len(tris)))
    assert len(tri) <= len(tris) + allowed
    assert (np.bincount(tri, minlength=len(tris)) >= 1).all() and (np.diff(tri) >= 0).all()
    total = np.cumsum(histogram(name)[0])
    assert 0 <= level < S.LEVELS and len(tri) == len(tris) + total[level]
    assert level == S.LEVELS - 1 or total[level + 1] > allowed  # the next level would not fit


@pytest.mark.parametrize("name", ["tiny0", "soup5000", "beams24x8"])
def test_budget_zero_is_the_unsplit_tree(name):
    tris, mats = triangles(name), materials(name)
    _, want = build_ploc(tris, mats)
    _, b = build_split(tris, mats, 0.0)
    assert same_bytes(b.nodes, want.nodes) and np.array_equal(b.tri_indices, want.tri_indices) and len(b.ref_boxes) == 0
    h = N.C.c_void_p()
    cfg = api.InstanceConfig().bvh_params()
    assert N.lib.adypt_bvh_build_ploc_split(api.Scene.FromArrays(tris, mats)._h, N.C.byref(cfg), 8, 0.0, N.C.byref(h), None) == N.ADYPT_OK
    p = N.C.c_void_p()
    n = N.lib.adypt_bvh_nodes(h, N.C.byref(p))
    assert n * 80 == len(want.nodes) and N.lib.adypt_bvh_ref_boxes(h, N.C.byref(p)) == 0 and not p
    N.lib.adypt_bvh_free(h)


def test_a_budget_under_which_nothing_splits_is_the_unsplit_tree():
    """300 copies of one triangle: every root cell is the scene's box, so the first level that splits any splits all 300, which 0.3 does not allow"""
    tris, mats = triangles("copies"), T.soup_material()
    level, tri, _ = lib_refs(tris, 0.3)
    assert len(tri) == len(tris) and level == 0
    _, want = build_ploc(tris, mats)
    _, b = build_split(tris, mats, 0.3)
    assert same_bytes(b.nodes, want.nodes) and np.array_equal(b.tri_indices, want.tri_indices) and len(b.ref_boxes) == 0


def test_determinism():
    tris, mats = triangles("beams24x8"), T.soup_material()
    a = build_split(tris, mats, 0.3)[1]
    for threads in (None, 1, 8):
        x = build_split(tris, mats, 0.3, threads=threads)[1]
        assert same_bytes(x.nodes, a.nodes) and np.array_equal(x.tri_indices, a.tri_indices) and np.array_equal(bits(x.ref_boxes), bits(a.ref_boxes))
    assert not same_bytes(a.nodes, build_ploc(tris, mats)[1].nodes) and len(a.tri_indices) > len(tris)


def as_triangles(ref_boxes):
    """one triangle per reference whose refit_triangle_box is the reference's box: the refit's restatement then bounds the references"""
    t = T.soup(len(ref_boxes), 1)
    t["p"][:, 0], t["p"][:, 1], t["p"][:, 2] = ref_boxes[:, :3], ref_boxes[:, 3:], ref_boxes[:, :3]
    return t


@pytest.mark.parametrize("budget", [0.3, 1.0])
@pytest.mark.parametrize("name", ["tiny0", "soup5000", "beams24x8"])
def test_boxes_and_refit(name, budget):
    tris, mats = triangles(name), materials(name)
    _, b = build_split(tris, mats, budget)
    level, tri, box = lib_refs(tris, budget)
    n_refs = len(tri)
    assert n_refs > len(tris) and len(b.tri_indices) == n_refs == len(b.ref_boxes) == b.build_info.refs and b.build_info.sbvh_nodes == 2 * n_refs - 1
    # the emitted references are the reference list, permuted: the same (triangle, box) pairs
    def pairs(t, bx):
        rows = np.concatenate([np.asarray(t, np.uint32)[:, None], bits(bx)], axis=1)
        return rows[np.lexsort(rows.T[::-1])]
    assert np.array_equal(pairs(b.tri_indices, b.ref_boxes), pairs(tri, box))
    n = np.ascontiguousarray(b.nodes).view(O.NODE_DT).reshape(-1)
    assert (L.leaf_order(n, b.tri_indices) == 1).all()
    # the node records are the refit's rule over the references' boxes, and every slot holds them in the node's frame
    want, lo, _, slo, shi = T.refit(b.nodes, np.arange(n_refs), as_triangles(b.ref_boxes))
    assert same_bytes(want, b.nodes) and T.slots_contain(b.nodes, lo, slo, shi)
    # refitted on the same triangles: a valid tree that bounds whole triangles (larger boxes, the same topology)
    r, again = lib_refit(b.nodes, b.tri_indices, tris)
    assert r == N.ADYPT_OK and not same_bytes(again, b.nodes)
    want, lo, _, slo, shi = T.refit(b.nodes, b.tri_indices, tris)
    assert same_bytes(again, want) and T.slots_contain(again, lo, slo, shi)
    m = np.ascontiguousarray(again).view(O.NODE_DT).reshape(-1)
    assert np.array_equal(m["meta"], n["meta"]) and np.array_equal(m["child_base"], n["child_base"]) and np.array_equal(m["tri_base"], n["tri_base"])


@pytest.mark.parametrize("pose", ["rest", "wave"])
@pytest.mark.parametrize("name", ["soup", "tiny0", "tiny1", "beams24x8"])
def test_hits_are_those_of_the_sbvh_tree(name, pose):
    """as tests/test_ploc_definition.py: t equal to the bit; tri_id may differ on at most 0.1 % of the rays, which are exact ties (t is equal)"""
    tris, mats = (rest(name) if not name.startswith("beams") else (triangles(name), T.soup_material()))
    moved = np.array(tris) if pose == "rest" else T.wave(tris)
    _, pb = build_split(moved, mats, 0.3)
    _, sb = build(moved, mats, 48)
    assert len(pb.tri_indices) > len(moved)
    rays = T.rays_in_box(moved, 50000)
    a, c = O.trace(O.Scene(pb.nodes, pb.tri_indices, moved, mats), rays), O.trace(O.Scene(sb.nodes, sb.tri_indices, moved, mats), rays)
    t_differs = bits(a["t"]) != bits(c["t"])
    id_differs = a["tri_id"] != c["tri_id"]
    print("%s %s: %d references of %d triangles; t differs on %d, tri_id on %d of %d rays; tris per ray split %.2f sbvh %.2f" % (
        name, pose, len(pb.tri_indices), len(moved), t_differs.sum(), id_differs.sum(), len(rays), a["tris"].mean(), c["tris"].mean()))
    if name.startswith("beams"):  # (the unsplit PLOC tree on the new fixture, for the record: inside the same allowance)
        _, ub = build_ploc(moved, mats)
        u = O.trace(O.Scene(ub.nodes, ub.tri_indices, moved, mats), rays)
        print("  unsplit ploc: t differs on %d, tri_id on %d" % ((bits(u["t"]) != bits(c["t"])).sum(), (u["tri_id"] != c["tri_id"]).sum()))
    assert t_differs.sum() == 0
    assert id_differs.sum() <= len(rays) // 1000
    assert (a["tri_id"] >= 0).any()


def leaf_area_ratio(ref_boxes):
    """the binary64 sum of the leaves' areas over the root's"""
    b = np.asarray(ref_boxes, np.float64)
    d = b[:, 3:] - b[:, :3]
    r = b[:, 3:].max(axis=0) - b[:, :3].min(axis=0)
    return (2 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])).sum() / (2 * (r[0] * r[1] + r[1] * r[2] + r[2] * r[0]))


def test_quality_with_long_thin_triangles():
    """beams(48, 24) at budget 0.3: the leaves' area at most half the unsplit tree's (a binary64 prototype gave 0.27 with random beams; the margin
    covers binary32, the pad and the deterministic beams), and through the oracle fewer triangle tests and fewer nodes per ray than the unsplit PLOC
    tree.  Measured here: leaf area / root area 16.33 unsplit, 4.16 split (ratio 0.255, 5 438 references); per ray 17.80 triangle tests and 7.08
    nodes unsplit, 2.76 and 7.04 split."""
    tris, mats = triangles("beams48x24"), T.soup_material()
    assert len(tris) == 4656
    p = S.positions(tris)
    whole = np.concatenate(S.boxes(p), axis=1)
    _, ub = build_ploc(tris, mats)
    _, sb = build_split(tris, mats, 0.3)
    assert len(tris) < len(sb.tri_indices) <= len(tris) + int(0.3 * len(tris))
    unsplit, split = leaf_area_ratio(whole), leaf_area_ratio(sb.ref_boxes)
    print("beams(48, 24): %d references; leaf area / root area unsplit %.2f split %.2f, ratio %.3f" % (len(sb.tri_indices), unsplit, split, split / unsplit))
    assert split <= 0.5 * unsplit
    rays = T.rays_in_box(tris, 20000)
    a, c = O.trace(O.Scene(sb.nodes, sb.tri_indices, tris, mats), rays), O.trace(O.Scene(ub.nodes, ub.tri_indices, tris, mats), rays)
    print("beams(48, 24): triangles per ray split %.2f unsplit %.2f; nodes per ray split %.2f unsplit %.2f" % (a["tris"].mean(), c["tris"].mean(), a["nodes"].mean(), c["nodes"].mean()))
    assert np.array_equal(bits(a["t"]), bits(c["t"]))
    assert a["tris"].mean() < c["tris"].mean() and a["nodes"].mean() < c["nodes"].mean()


def test_refusals():
    tris, mats = rest("tiny2")
    sc = api.Scene.FromArrays(tris, mats)
    cfg = api.InstanceConfig().bvh_params()
    h = N.C.c_void_p()
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    for budget in (-0.1, 1.5, float("nan")):
        assert N.lib.adypt_bvh_build_ploc_split(sc._h, N.C.byref(cfg), 8, budget, N.C.byref(h), None) == N.E_INVALID and not h
        assert N.lib.adypt_presplit_refs(t.ctypes.data, len(tris), budget, 0, None, None, None) == N.E_INVALID
    assert N.lib.adypt_bvh_build_ploc_split(None, N.C.byref(cfg), 8, 0.3, N.C.byref(h), None) == N.E_INVALID and not h
    assert N.lib.adypt_presplit_refs(None, 5, 0.3, 0, None, None, None) == N.E_INVALID
    assert N.lib.adypt_bvh_build_ploc_split(sc._h, N.C.byref(cfg), 0, 0.3, N.C.byref(h), None) == N.E_INVALID and not h
    broken = np.array(tris)
    broken["p"][1, 0] = np.nan  # a NaN vertex
    assert N.lib.adypt_bvh_build_ploc_split(api.Scene.FromArrays(broken, mats)._h, N.C.byref(cfg), 8, 0.3, N.C.byref(h), None) == N.E_INVALID and not h
    assert N.lib.adypt_presplit_refs(np.ascontiguousarray(broken).view(np.uint8).ctypes.data, len(tris), 0.3, 0, None, None, None) == N.E_INVALID
    assert N.lib.adypt_bvh_build_ploc_split(sc._h, N.C.byref(cfg), 8, 0.3, N.C.byref(h), None) == N.ADYPT_OK and h
    N.lib.adypt_bvh_free(h)
