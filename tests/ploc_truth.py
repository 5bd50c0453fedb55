"""The pairing of the PLOC builder (adypt_amd/csrc/device/ploc.hpp) restated in numpy float32, a round at a time over whole arrays: the same scan order
(ascending j, strict <, +inf to start from), the same merge rule and the same ids.  Boxes are kept as the integer keys that order the binary32 values
(tests/refit_truth.py), so a union is the definition's refit_min / refit_max whatever the order."""
import numpy as np

from oracle import oracle_py as O
from tests import lbvh_truth as L
from tests import refit_truth as T


def area(lo_key, hi_key):
    """cut_area of boxes given as keys: (ex * (ey + ez) + ey * ez) * 2 in binary32, the operations in that order"""
    with np.errstate(invalid="ignore", over="ignore"):
        e = (T.unkey(hi_key) - T.unkey(lo_key)).astype(np.float32)
        s = (e[..., 1] + e[..., 2]).astype(np.float32)
        a = (e[..., 0] * s).astype(np.float32)
        b = (e[..., 1] * e[..., 2]).astype(np.float32)
        return ((a + b).astype(np.float32) * np.float32(2.0)).astype(np.float32)


def leaf_boxes(triangles):
    """(lo, hi) keys [n, 3] of the triangles' boxes in sorted key order, and that order"""
    order = L.sorted_order(triangles)
    p = np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1)["p"].astype(np.float32)[order]
    k = T.key(p)
    return k.min(axis=1), k.max(axis=1), order


def tree(triangles, radius):
    """(left, right, rounds): int32 [n - 1] each, the children of the inner nodes in the ids of lbvh.hpp"""
    lo, hi, _ = leaf_boxes(triangles)
    n = len(lo)
    left, right = np.zeros(max(n - 1, 0), np.int32), np.zeros(max(n - 1, 0), np.int32)
    cluster = np.arange(n, dtype=np.int64) + (n - 1)
    nxt, rounds = n - 1, 0
    while len(cluster) > 1:
        m = len(cluster)
        idx = np.arange(m)
        best, pick = np.full(m, np.inf, np.float32), np.full(m, -1, np.int64)
        for off in list(range(-radius, 0)) + list(range(1, radius + 1)):
            j = idx + off
            ok = (j >= 0) & (j < m)
            jj = np.clip(j, 0, m - 1)
            d = area(np.minimum(lo, lo[jj]), np.maximum(hi, hi[jj]))
            better = ok & (d < best)
            best, pick = np.where(better, d, best), np.where(better, jj, pick)
        mutual = (pick >= 0) & (pick[np.clip(pick, 0, m - 1)] == idx)
        lower = np.nonzero(mutual & (idx < pick))[0]
        k = len(lower)
        assert k > 0, "a round merged nothing"
        upper = pick[lower]
        ids = nxt - k + np.arange(k)
        left[ids], right[ids] = cluster[lower], cluster[upper]
        cluster[lower] = ids
        lo[lower], hi[lower] = np.minimum(lo[lower], lo[upper]), np.maximum(hi[lower], hi[upper])
        keep = np.ones(m, bool)
        keep[upper] = False
        cluster, lo, hi = cluster[keep], lo[keep], hi[keep]
        nxt -= k
        rounds += 1
    assert nxt == 0
    return left, right, rounds


def leaf_sets(left, right, n):
    """per node id (2 n - 1): the frozenset of sorted positions below it"""
    sets = [None] * (2 * n - 1)
    for j in range(n):
        sets[n - 1 + j] = frozenset((j,))
    for i in sorted(range(n - 1), reverse=True):  # (children of a PLOC node carry higher ids: built in earlier rounds, or leaves)
        sets[i] = sets[left[i]] | sets[right[i]]
    return sets


def inner_area(triangles, left, right):
    """(sum of the inner nodes' areas, the root's area) in binary64, from exact leaf boxes"""
    _, _, order = leaf_boxes(triangles)
    p = np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1)["p"].astype(np.float64)[order]
    n = len(p)
    lo, hi = np.zeros((2 * n - 1, 3)), np.zeros((2 * n - 1, 3))
    lo[n - 1:], hi[n - 1:] = p.min(axis=1), p.max(axis=1)
    done = np.zeros(2 * n - 1, bool)
    done[n - 1:] = True
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    while not done[:n - 1].all():
        ready = np.nonzero(~done[:n - 1] & done[left] & done[right])[0]
        assert len(ready)
        lo[ready], hi[ready] = np.minimum(lo[left[ready]], lo[right[ready]]), np.maximum(hi[left[ready]], hi[right[ready]])
        done[ready] = True
    d = hi - lo
    a = 2 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])
    return a[:n - 1].sum(), a[0]
