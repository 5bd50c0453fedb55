"""The keys of the linear BVH (adypt_amd/csrc/device/lbvh.hpp) restated in numpy float32, whole arrays at a time, and what the tests of the linear
builder ask of a tree.  The centroid box is taken on integer keys that order the binary32 values (tests/refit_truth.py), so it is the definition's
refit_min / refit_max whatever the order."""
import numpy as np

from oracle import oracle_py as O
from tests import refit_truth as T


def centroids(triangles):
    p = np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1)["p"].astype(np.float32)   # [T, vertex, axis]
    s = (p[:, 0] + p[:, 1]).astype(np.float32)
    s = (s + p[:, 2]).astype(np.float32)
    return (s * np.float32(1.0 / 3)).astype(np.float32)


def cells(triangles):
    c = centroids(triangles)
    lo, hi = T.unkey(T.key(c).min(axis=0)), T.unkey(T.key(c).max(axis=0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scale = (np.float32(1024.0) / (hi - lo).astype(np.float32)).astype(np.float32)
        q = ((c - lo).astype(np.float32) * scale).astype(np.float32)
        ok = (q > 0) & np.isfinite(q)
        return np.where(ok, np.minimum(np.where(ok, q, 0), 1023).astype(np.int64), 0).astype(np.uint64)


def spread(v):
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def keys(triangles):
    """uint64 [T]: Morton code << 32 | triangle index, x the highest bit of every triple"""
    q = cells(triangles)
    code = spread(q[:, 0]) << np.uint64(2) | spread(q[:, 1]) << np.uint64(1) | spread(q[:, 2])
    return code << np.uint64(32) | np.arange(len(q), dtype=np.uint64)


def sorted_order(triangles):
    """the triangle indices in the order of their keys"""
    return (np.sort(keys(triangles)) & np.uint64(0xffffffff)).astype(np.int64)


def leaf_order(nodes, tri_indices):
    """The triangles as a depth-first walk of the wide tree meets them when it takes the slots' references in the order they lie in tri_indices: every
    node's own references are one run, its subtrees' follow — so this is tri_indices itself, and the check is that every run is where the walk
    expects it."""
    n = np.ascontiguousarray(nodes).view(O.NODE_DT).reshape(-1)
    _, inner, child, leaf, first, count = T.decode(n)
    seen = np.zeros(len(tri_indices), dtype=np.int64)
    for r in range(3):
        m = count > r
        np.add.at(seen, first[m] + r, 1)
    return seen


def check_tree(nodes, tri_indices, n_tris):
    """a valid tree over n_tris triangles without splits: every reference in exactly one leaf slot, tri_indices a permutation, leaves of 1..3 references
    at offsets below 24"""
    n = np.ascontiguousarray(nodes).view(O.NODE_DT).reshape(-1)
    idx = np.asarray(tri_indices)
    assert len(idx) == n_tris and np.array_equal(np.sort(idx), np.arange(n_tris))
    _, inner, _, leaf, first, count = T.decode(n)
    assert ((count[leaf] >= 1) & (count[leaf] <= 3)).all()
    off = (n["meta"].astype(np.int64) & 31)[leaf]
    assert (off + count[leaf] <= 24).all()
    assert (leaf_order(n, idx) == 1).all()
    T.depths(n)  # every node reached once
