"""The linear BVH on the host: adypt_bvh_build_linear (csrc/device/lbvh.hpp + wide_cut.hpp + refit.hpp) against the numpy restatement of its keys
(tests/lbvh_truth.py), against the refit, and against the SBVH builder's tree through the CPU oracle.  No GPU."""
import functools

import numpy as np
import pytest

from adypt_amd import _native as N
from adypt_amd import api
from oracle import oracle_py as O
from tests import lbvh_truth as L
from tests import refit_truth as T
from tests.helpers import bits
from tests.test_refit_definition import build, flat_scene, lib_refit, rest, same_bytes

SCENES = ("tiny0", "tiny1", "tiny2", "soup")


def build_linear(tris, mats, threads=None):
    sc = api.Scene.FromArrays(tris, mats)
    b = api.WideBVH()
    if threads is not None:
        N.lib.adypt_host_set_threads(threads)
    try:
        b.BuildLinear(sc, api.InstanceConfig().bvh_params())
    finally:
        if threads is not None:
            N.lib.adypt_host_set_threads(0)
    return sc, b


@functools.lru_cache(maxsize=None)
def linear(name):
    return build_linear(*rest(name))


@pytest.mark.parametrize("name", SCENES)
def test_valid_tree_and_fixed_point_of_the_refit(name):
    tris, _ = rest(name)
    _, b = linear(name)
    L.check_tree(b.nodes, b.tri_indices, len(tris))
    r, again = lib_refit(b.nodes, b.tri_indices, tris)  # (OK: plan_refit accepts the arrays)
    assert r == N.ADYPT_OK and same_bytes(again, b.nodes)
    want, lo, _, slo, shi = T.refit(b.nodes, b.tri_indices, tris)
    assert same_bytes(want, b.nodes) and T.slots_contain(b.nodes, lo, slo, shi)
    assert b.build_info.refs == len(tris) and b.build_info.sbvh_nodes == 2 * len(tris) - 1 and b.build_info.wide_nodes == len(b.nodes) // 80


def leaves_in_walk_order(nodes, tri_indices):
    """the triangles in the order of a depth-first walk that takes a node's slots by ascending first Morton position: for a tree cut from a radix tree
    over sorted keys every subtree is a contiguous range of the sorted order, so the SET of every node's references is such a range"""
    n = np.ascontiguousarray(nodes).view(O.NODE_DT).reshape(-1)
    _, inner, child, leaf, first, count = T.decode(n)
    return n, inner, child, leaf, first, count


@pytest.mark.parametrize("name", SCENES)
def test_keys_against_numpy(name):
    tris, _ = rest(name)
    _, b = linear(name)
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    got = np.zeros(len(tris), dtype=np.uint64)
    assert N.lib.adypt_lbvh_keys(t.ctypes.data, len(tris), got.ctypes.data) == N.ADYPT_OK
    assert np.array_equal(got, np.sort(L.keys(tris))), "the library's sorted keys"
    order = L.sorted_order(tris)
    rank = np.empty(len(tris), dtype=np.int64)
    rank[order] = np.arange(len(tris))
    # every subtree of a radix tree over the sorted keys covers a contiguous range of the sorted order — and so does every leaf slot and every node
    n, inner, child, leaf, first, count = leaves_in_walk_order(b.nodes, b.tri_indices)
    idx = np.asarray(b.tri_indices, dtype=np.int64)
    r = rank[idx]
    for k in (2, 3):
        m = leaf & (count == k)
        runs = np.stack([r[first[m] + j] for j in range(k)], axis=1)
        assert (runs.max(axis=1) - runs.min(axis=1) == k - 1).all(), "a leaf slot of %d references is no range of the sorted order" % k
    depth = T.depths(n)
    lo = np.full(len(n), len(tris), dtype=np.int64)
    hi = np.full(len(n), -1, dtype=np.int64)
    cnt = np.zeros(len(n), dtype=np.int64)
    for d in range(int(depth.max()), -1, -1):
        for i in np.nonzero(depth == d)[0]:
            for s in range(8):
                if leaf[i, s]:
                    rr = r[first[i, s]:first[i, s] + count[i, s]]
                    lo[i], hi[i], cnt[i] = min(lo[i], rr.min()), max(hi[i], rr.max()), cnt[i] + len(rr)
                elif inner[i, s]:
                    c = child[i, s]
                    lo[i], hi[i], cnt[i] = min(lo[i], lo[c]), max(hi[i], hi[c]), cnt[i] + cnt[c]
    assert (hi - lo + 1 == cnt).all(), "a node's references are no range of the sorted order"
    assert cnt[0] == len(tris)
    # the keys themselves: cells inside 10 bits, and the degenerate rules
    q = L.cells(tris)
    c = L.centroids(tris)
    extent = c.max(axis=0) > c.min(axis=0)
    assert (q.min(axis=0) == 0).all() and (q.max(axis=0)[extent] == 1023).all() and (q.max(axis=0)[~extent] == 0).all()


def test_determinism():
    tris, mats = rest("soup")
    a = build_linear(tris, mats)[1]
    b = build_linear(tris, mats)[1]
    one = build_linear(tris, mats, threads=1)[1]
    eight = build_linear(tris, mats, threads=8)[1]
    for x in (b, one, eight):
        assert same_bytes(x.nodes, a.nodes) and np.array_equal(x.tri_indices, a.tri_indices)


def shared_centroid(n, seed):
    """n different triangles with one centroid: vertices c + d, c + e, c - d - e in exactly representable numbers"""
    rs = np.random.RandomState(seed)
    t = T.soup(n, seed)
    c = np.array([2.0, -4.0, 8.0], dtype=np.float32)
    d, e = rs.randint(-64, 65, size=(n, 3)).astype(np.float32) / 16, rs.randint(-64, 65, size=(n, 3)).astype(np.float32) / 16
    t["p"][:, 0], t["p"][:, 1], t["p"][:, 2] = c + d, c + e, c - d - e
    return t


DEGENERATE = {
    "one": lambda: T.soup(1, 3),
    "two": lambda: T.soup(2, 4),
    "shared_centroid": lambda: shared_centroid(300, 6),
    "flat": lambda: flat_scene(40, 1),
    "257": lambda: T.soup(257, 9),
}


@pytest.mark.parametrize("what", sorted(DEGENERATE))
def test_degenerate_inputs(what):
    tris, mats = DEGENERATE[what](), T.soup_material()
    _, b = build_linear(tris, mats)
    L.check_tree(b.nodes, b.tri_indices, len(tris))
    assert same_bytes(lib_refit(b.nodes, b.tri_indices, tris)[1], b.nodes)
    if what == "shared_centroid":
        c = L.centroids(tris)
        assert (c == c[0]).all() and (L.cells(tris) == 0).all()  # one centroid: every cell 0, the index alone orders the keys
        assert np.array_equal(L.sorted_order(tris), np.arange(len(tris)))
    if what == "flat":
        assert (L.cells(tris)[:, 2] == 0).all()
    if what == "one":
        n = np.ascontiguousarray(b.nodes).view(O.NODE_DT)
        assert len(n) == 1 and list(n["meta"][0] >> 5).count(1) == 1
    # rays at the triangles' own centroids from outside: every one hits something through the tree, and what it hits is what a brute-force tree-free
    # reference (the one-node-per-three-triangles SBVH of the same scene) hits
    sc = O.Scene(b.nodes, b.tri_indices, tris, mats)
    target = L.centroids(tris).astype(np.float64) if what != "shared_centroid" else tris["p"][:, 0].astype(np.float64) * 0.25 + L.centroids(tris) * 0.75
    rays = np.zeros((len(tris), 8), np.float32)
    origin = np.array([37.0, 41.0, 43.0])
    rays[:, :3], rays[:, 3], rays[:, 4:7] = origin, 1e-4, target - origin
    got = O.trace(sc, rays)
    _, ref_bvh = build(tris, mats, -1)
    want = O.trace(O.Scene(ref_bvh.nodes, ref_bvh.tri_indices, tris, mats), rays)
    assert np.array_equal(bits(got["t"]), bits(want["t"]))
    assert (got["tri_id"] >= 0).sum() >= max(1, len(tris) // 2)


@pytest.mark.parametrize("pose", ["rest", "wave"])
@pytest.mark.parametrize("name", ["soup", "tiny0", "tiny1"])
def test_hits_are_those_of_the_sbvh_tree(name, pose):
    tris, mats = rest(name)
    moved = np.array(tris) if pose == "rest" else T.wave(tris)
    _, lb = build_linear(moved, mats)
    _, sb = build(moved, mats, 48)
    rays = T.rays_in_box(moved, 50000)
    a, c = O.trace(O.Scene(lb.nodes, lb.tri_indices, moved, mats), rays), O.trace(O.Scene(sb.nodes, sb.tri_indices, moved, mats), rays)
    t_differs = bits(a["t"]) != bits(c["t"])
    id_differs = a["tri_id"] != c["tri_id"]
    print("%s %s: t differs on %d, tri_id on %d of %d rays; nodes per ray linear %.2f sbvh %.2f" % (name, pose, t_differs.sum(), id_differs.sum(), len(rays), a["nodes"].mean(), c["nodes"].mean()))
    assert t_differs.sum() == 0
    assert id_differs.sum() <= len(rays) // 1000  # (only exact ties: t is equal everywhere)
    assert (a["tri_id"] >= 0).any()


def test_refusals():
    tris, mats = rest("tiny2")
    sc = api.Scene.FromArrays(tris, mats)
    for tri_sah, node_sah in ((0.0, 1.0), (0.3, -1.0), (float("nan"), 1.0), (0.3, float("inf"))):
        cfg = api.InstanceConfig().bvh_params()
        cfg.triangle_sah, cfg.node_sah = tri_sah, node_sah
        h = N.C.c_void_p()
        assert N.lib.adypt_bvh_build_linear(sc._h, N.C.byref(cfg), N.C.byref(h), None) == N.E_INVALID and not h
    assert N.lib.adypt_bvh_build_linear(None, None, None, None) == N.E_INVALID
