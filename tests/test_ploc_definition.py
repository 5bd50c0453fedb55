"""The PLOC tree on the host: adypt_ploc_tree and adypt_bvh_build_ploc (csrc/device/ploc.hpp + wide_cut.hpp + refit.hpp) against the numpy restatement of the
pairing (tests/ploc_truth.py), against the refit, against the SBVH builder's tree through the CPU oracle, and against the radix tree of the linear
builder in what the tree is for: less area, fewer nodes per ray — on a mesh; no claim is made on a triangle soup.  No GPU."""
import functools

import numpy as np
import pytest

from adypt_amd import _native as N
from adypt_amd import api
from oracle import oracle_py as O
from tests import lbvh_truth as L
from tests import ploc_truth as P
from tests import refit_truth as T
from tests.helpers import bits
from tests.test_lbvh_definition import build_linear, shared_centroid
from tests.test_refit_definition import build, lib_refit, rest, same_bytes

RADII = (1, 8, 32)


@functools.lru_cache(maxsize=None)
def triangles(name):
    return T.soup(5000) if name == "soup5000" else rest(name)[0]


def lib_tree(tris, radius):
    """adypt_ploc_tree: (code, left, right)"""
    n = len(tris)
    left, right = np.full(max(n - 1, 1), -7, np.int32), np.full(max(n - 1, 1), -7, np.int32)
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    r = N.lib.adypt_ploc_tree(t.ctypes.data, n, radius, left.ctypes.data, right.ctypes.data)
    return r, left[:n - 1], right[:n - 1]


def build_ploc(tris, mats, radius=8, threads=None):
    sc = api.Scene.FromArrays(tris, mats)
    b = api.WideBVH()
    if threads is not None:
        N.lib.adypt_host_set_threads(threads)
    try:
        b.BuildPLOC(sc, api.InstanceConfig().bvh_params(), radius)
    finally:
        if threads is not None:
            N.lib.adypt_host_set_threads(0)
    return sc, b


def materials(name):
    return T.soup_material() if name == "soup5000" else rest(name)[1]


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", ["tiny0", "tiny1", "tiny2", "soup5000"])
def test_library_tree_equals_numpy(name, radius):
    tris = triangles(name)
    r, left, right = lib_tree(tris, radius)
    assert r == N.ADYPT_OK
    want_left, want_right, rounds = P.tree(tris, radius)
    print("%s radius %d: %d rounds for %d triangles" % (name, radius, rounds, len(tris)))
    assert np.array_equal(left, want_left) and np.array_equal(right, want_right)


def reference_sets(nodes, tri_indices, rank):
    """per wide node: the frozenset of the sorted positions of every reference below it"""
    n = np.ascontiguousarray(nodes).view(O.NODE_DT).reshape(-1)
    _, inner, child, leaf, first, count = T.decode(n)
    depth = T.depths(n)
    idx = np.asarray(tri_indices, dtype=np.int64)
    sets = [None] * len(n)
    for i in np.argsort(-depth, kind="stable"):
        s = set()
        for k in range(8):
            if leaf[i, k]:
                s.update(int(x) for x in rank[idx[first[i, k]:first[i, k] + count[i, k]]])
            elif inner[i, k]:
                s |= sets[child[i, k]]
        sets[i] = frozenset(s)
    return sets


@pytest.mark.parametrize("name", ["tiny0", "tiny1", "tiny2", "soup5000"])
def test_valid_tree_and_fixed_point_of_the_refit(name):
    tris, mats = triangles(name), materials(name)
    _, b = build_ploc(tris, mats)
    L.check_tree(b.nodes, b.tri_indices, len(tris))
    assert len(b.tri_indices) == len(tris) and np.array_equal(np.sort(b.tri_indices), np.arange(len(tris)))
    r, again = lib_refit(b.nodes, b.tri_indices, tris)
    assert r == N.ADYPT_OK and same_bytes(again, b.nodes)
    want, lo, _, slo, shi = T.refit(b.nodes, b.tri_indices, tris)
    assert same_bytes(want, b.nodes) and T.slots_contain(b.nodes, lo, slo, shi)
    assert b.build_info.refs == len(tris) and b.build_info.sbvh_nodes == 2 * len(tris) - 1 and b.build_info.wide_nodes == len(b.nodes) // 80
    # every wide node holds exactly the leaves of one node of the numpy binary tree
    left, right, _ = P.tree(tris, 8)
    binary = set(P.leaf_sets(left, right, len(tris)))
    order = L.sorted_order(tris)
    rank = np.empty(len(tris), dtype=np.int64)
    rank[order] = np.arange(len(tris))
    wide = reference_sets(b.nodes, b.tri_indices, rank)
    assert len(wide[0]) == len(tris) and all(s in binary for s in wide)


def test_determinism():
    tris, mats = triangles("soup5000"), T.soup_material()
    a = build_ploc(tris, mats)[1]
    for threads in (None, 1, 8):
        x = build_ploc(tris, mats, threads=threads)[1]
        assert same_bytes(x.nodes, a.nodes) and np.array_equal(x.tri_indices, a.tri_indices)
    assert not same_bytes(a.nodes, build_linear(tris, mats)[1].nodes)  # (another tree than the linear one)
    assert not same_bytes(a.nodes, build_ploc(tris, mats, radius=1)[1].nodes)


@pytest.mark.parametrize("pose", ["rest", "wave"])
@pytest.mark.parametrize("name", ["soup", "tiny0", "tiny1"])
def test_hits_are_those_of_the_sbvh_tree(name, pose):
    """as tests/test_lbvh_definition.py: t equal to the bit; tri_id may differ on at most 0.1 % of the rays, which are exact ties (t is equal)"""
    tris, mats = rest(name)
    moved = np.array(tris) if pose == "rest" else T.wave(tris)
    _, pb = build_ploc(moved, mats)
    _, sb = build(moved, mats, 48)
    rays = T.rays_in_box(moved, 50000)
    a, c = O.trace(O.Scene(pb.nodes, pb.tri_indices, moved, mats), rays), O.trace(O.Scene(sb.nodes, sb.tri_indices, moved, mats), rays)
    t_differs = bits(a["t"]) != bits(c["t"])
    id_differs = a["tri_id"] != c["tri_id"]
    print("%s %s: t differs on %d, tri_id on %d of %d rays; nodes per ray ploc %.2f sbvh %.2f" % (name, pose, t_differs.sum(), id_differs.sum(), len(rays), a["nodes"].mean(), c["nodes"].mean()))
    assert t_differs.sum() == 0
    assert id_differs.sum() <= len(rays) // 1000
    assert (a["tri_id"] >= 0).any()


def height_field(m=48):
    """2 m m triangles of y = 1.5 sin(0.7 x) + 0.8 cos(0.9 z) over [-10, 10]^2, and two wall triangles behind them: a structured mesh"""
    x, z = np.meshgrid(np.linspace(-10, 10, m + 1), np.linspace(-10, 10, m + 1), indexing="ij")
    y = 1.5 * np.sin(0.7 * x) + 0.8 * np.cos(0.9 * z)
    g = np.stack([x, y, z], -1)
    a, b, c, d = g[:-1, :-1], g[1:, :-1], g[:-1, 1:], g[1:, 1:]
    p = np.concatenate([np.stack([a, b, c], 2).reshape(-1, 3, 3), np.stack([b, d, c], 2).reshape(-1, 3, 3)])
    wall = np.array([[[-10, -3, -10], [10, -3, -10], [10, 5, -10]], [[-10, -3, -10], [10, 5, -10], [-10, 5, -10]]], float)
    p = np.concatenate([p, wall]).astype(np.float32)
    t = T.soup(len(p), 5)
    t["p"] = p
    return t


def radix_tree(tris):
    """(left, right) of the radix tree over the sorted keys, in the ids of lbvh.hpp: a range splits where the highest differing bit of its first and last
    key changes, and the inner node of a range is the end of it that borders the split (Karras 2012)"""
    keys = np.sort(L.keys(tris))
    n = len(keys)
    left, right = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32)
    todo = [(0, n - 1, 0)]
    while todo:
        a, b, me = todo.pop()
        bit = (int(keys[a]) ^ int(keys[b])).bit_length() - 1
        s = int(np.searchsorted(keys[a:b + 1], np.uint64((int(keys[b]) >> bit) << bit))) + a  # the first key of the upper half
        for first, last, out, inner in ((a, s - 1, left, s - 1), (s, b, right, s)):
            out[me] = n - 1 + first if first == last else inner
            if first != last:
                todo.append((first, last, inner))
    return left, right


def test_quality_on_a_structured_mesh():
    """The sum of the inner nodes' areas over the root's (the SAH's node term): at radius 8 at most 0.8 of the radix tree's — a numpy prototype in binary64
    gave 0.65 to 0.70 on this construction at 290 and 45 002 triangles, the margin covers binary32 — and, after the collapse, fewer nodes per ray."""
    tris, mats = height_field(), T.soup_material()
    assert len(tris) == 2 * 48 * 48 + 2
    r, left, right = lib_tree(tris, 8)
    assert r == N.ADYPT_OK
    rl, rr = radix_tree(tris)
    assert np.array_equal(np.sort(np.concatenate([rl, rr])), np.arange(1, 2 * len(tris) - 1))  # every node but the root is one node's child
    ploc, root = P.inner_area(tris, left, right)
    radix, _ = P.inner_area(tris, rl, rr)
    print("height field, %d triangles: inner area / root area: ploc %.2f, radix tree %.2f, ratio %.3f" % (len(tris), ploc / root, radix / root, ploc / radix))
    assert ploc <= 0.8 * radix
    rays = T.rays_in_box(tris, 20000)
    _, pb = build_ploc(tris, mats)
    _, lb = build_linear(tris, mats)
    a, c = O.trace(O.Scene(pb.nodes, pb.tri_indices, tris, mats), rays), O.trace(O.Scene(lb.nodes, lb.tri_indices, tris, mats), rays)
    print("height field: nodes per ray ploc %.2f linear %.2f; triangles per ray ploc %.2f linear %.2f" % (a["nodes"].mean(), c["nodes"].mean(), a["tris"].mean(), c["tris"].mean()))
    assert np.array_equal(bits(a["t"]), bits(c["t"]))
    assert a["nodes"].mean() < c["nodes"].mean()


def copies(n):
    t = T.soup(n, 8)
    t["p"][:] = t["p"][0]
    return t


DEGENERATE = {
    "one": lambda: T.soup(1, 3),
    "two": lambda: T.soup(2, 4),
    "radius_plus_one": lambda: T.soup(9, 5),
    "shared_centroid": lambda: shared_centroid(300, 6),
    "copies": lambda: copies(300),
}


@pytest.mark.parametrize("what", sorted(DEGENERATE))
def test_degenerate_inputs(what):
    tris, mats = DEGENERATE[what](), T.soup_material()
    r, left, right = lib_tree(tris, 8)
    assert r == N.ADYPT_OK
    want_left, want_right, _ = P.tree(tris, 8)
    assert np.array_equal(left, want_left) and np.array_equal(right, want_right)
    assert len(P.leaf_sets(left, right, len(tris))[0]) == len(tris)  # one tree over every leaf
    _, b = build_ploc(tris, mats)
    L.check_tree(b.nodes, b.tri_indices, len(tris))
    assert same_bytes(lib_refit(b.nodes, b.tri_indices, tris)[1], b.nodes)
    if what == "one":
        n = np.ascontiguousarray(b.nodes).view(O.NODE_DT)
        assert len(n) == 1 and list(n["meta"][0] >> 5).count(1) == 1
    if what == "copies":
        assert np.array_equal(L.sorted_order(tris), np.arange(len(tris)))
    # rays at the triangles from outside hit what they hit through the SBVH builder's unsplit tree
    sc = O.Scene(b.nodes, b.tri_indices, tris, mats)
    p = tris["p"].astype(np.float64)
    target = p[:, 0] * 0.25 + p.mean(axis=1) * 0.75
    rays = np.zeros((len(tris), 8), np.float32)
    origin = np.array([37.0, 41.0, 43.0])
    rays[:, :3], rays[:, 3], rays[:, 4:7] = origin, 1e-4, target - origin
    got = O.trace(sc, rays)
    _, ref_bvh = build(tris, mats, -1)
    want = O.trace(O.Scene(ref_bvh.nodes, ref_bvh.tri_indices, tris, mats), rays)
    assert np.array_equal(bits(got["t"]), bits(want["t"]))
    assert (got["tri_id"] >= 0).sum() >= max(1, len(tris) // 2)


def test_refusals():
    tris, mats = rest("tiny2")
    sc = api.Scene.FromArrays(tris, mats)
    cfg = api.InstanceConfig().bvh_params()
    h = N.C.c_void_p()
    for radius in (0, 33, -1):
        assert N.lib.adypt_bvh_build_ploc(sc._h, N.C.byref(cfg), radius, N.C.byref(h), None) == N.E_INVALID and not h
        assert lib_tree(tris, radius)[0] == N.E_INVALID
    for tri_sah, node_sah in ((0.0, 1.0), (0.3, -1.0), (float("nan"), 1.0), (0.3, float("inf"))):
        bad = api.InstanceConfig().bvh_params()
        bad.triangle_sah, bad.node_sah = tri_sah, node_sah
        assert N.lib.adypt_bvh_build_ploc(sc._h, N.C.byref(bad), 8, N.C.byref(h), None) == N.E_INVALID and not h
    assert N.lib.adypt_bvh_build_ploc(None, None, 8, None, None) == N.E_INVALID
    broken = np.array(tris)
    broken["p"][1, 0] = np.nan  # a NaN vertex
    assert lib_tree(broken, 8)[0] == N.E_INVALID
    assert N.lib.adypt_bvh_build_ploc(api.Scene.FromArrays(broken, mats)._h, N.C.byref(cfg), 8, N.C.byref(h), None) == N.E_INVALID and not h
    assert N.lib.adypt_bvh_build_ploc(sc._h, N.C.byref(cfg), 8, N.C.byref(h), None) == N.ADYPT_OK and h
    N.lib.adypt_bvh_free(h)
