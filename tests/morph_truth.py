"""Morph targets in front of the matrices (adypt_amd/csrc/device/pose.hpp, the header's opening comment) restated in numpy float32, whole arrays at a time:
what adypt_pose_triangles_morph and the device path (BindMorph, Pose(morph_weights=...)) are held against, bit for bit.  Written from the definition, not
from the header's loops: the entries are ranked per triangle by target index, and rank r of every triangle is applied at once — one binary32 product and
one binary32 sum per word, an entry of weight 0 skipped.  Then tests/pose_truth.py poses the morphed triangles."""
import numpy as np

from oracle import oracle_py as O
from tests import pose_truth as P

F = np.float32


def morph(triangles, entry_triangles, entry_targets, deltas, morph_weights):
    """the TRI_DT triangles after the morph stage alone"""
    t = np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1).copy()
    n = len(t)
    tri = np.asarray(entry_triangles, dtype=np.int64).reshape(-1)
    tgt = np.asarray(entry_targets, dtype=np.int64).reshape(-1)
    d = np.ascontiguousarray(deltas, dtype=F).reshape(-1, 18)
    w = np.ascontiguousarray(morph_weights, dtype=F).reshape(-1)
    acc = np.concatenate([t["p"].reshape(n, 9), t["n"].reshape(n, 9)], axis=1).astype(F)   # words 0..17
    order = np.lexsort((tgt, tri))                                                         # by triangle, then by target
    tri, tgt, d = tri[order], tgt[order], d[order]
    first = np.searchsorted(tri, tri, side="left")
    rank = np.arange(len(tri)) - first                                                     # the entry's place among its triangle's
    for r in range(int(rank.max()) + 1 if len(rank) else 0):
        use = (rank == r) & (w[tgt] != 0)                                                  # a triangle at most once per rank
        product = (w[tgt[use]][:, None] * d[use]).astype(F)
        acc[tri[use]] = (acc[tri[use]] + product).astype(F)
    t["p"], t["n"] = acc[:, :9].reshape(n, 3, 3), acc[:, 9:].reshape(n, 3, 3)
    return t


def pose(triangles, matrices, entries, morph_weights, parts=None, joints=None, weights=None):
    """rest pose -> morph -> vertex matrix: the posed TRI_DT triangles"""
    return P.pose(morph(triangles, *entries, morph_weights), matrices, parts=parts, joints=joints, weights=weights)


# ---- layers the tests share ----
def entries_of(n, n_targets, seed=13):
    """(triangles int32 [e], targets int32 [e], deltas float32 [e, 18]) in a shuffled order.  With five triangles or more: triangle 0 has no entry,
    triangles 1, 2 and 3 have 1, 2 and min(n_targets, 12) entries, triangle 4 one for every target; the last triangle always has entries (with fewer
    than five triangles it has one for every target); about a third of the others have one to four."""
    rs = np.random.RandomState(seed + n + 7 * n_targets)
    per_tri = {}
    for i in range(5, n - 1):
        if rs.uniform() < 0.3:
            per_tri[i] = rs.choice(n_targets, size=min(n_targets, rs.randint(1, 5)), replace=False)
    if n >= 5:
        per_tri[1] = rs.choice(n_targets, size=1, replace=False)
        per_tri[2] = rs.choice(n_targets, size=min(n_targets, 2), replace=False)
        per_tri[3] = rs.choice(n_targets, size=min(n_targets, 12), replace=False)
        per_tri[4] = np.arange(n_targets)
        per_tri[n - 1] = rs.choice(n_targets, size=min(n_targets, 3), replace=False)
    else:
        per_tri[n - 1] = np.arange(n_targets)
    tri = np.concatenate([np.full(len(k), i) for i, k in per_tri.items()]).astype(np.int32)
    tgt = np.concatenate(list(per_tri.values())).astype(np.int32)
    d = rs.normal(0.0, 0.1, size=(len(tri), 18)).astype(F)
    shuffle = rs.permutation(len(tri))
    return tri[shuffle], tgt[shuffle], np.ascontiguousarray(d[shuffle])


def weights_of(n_targets, seed=17):
    """float32 [n_targets] in [-1, 1.5], negative ones among them; from three targets on every third is 0, so that active and skipped entries
    interleave on a triangle that has an entry for every target"""
    w = np.random.RandomState(seed + n_targets).uniform(-1.0, 1.5, size=n_targets).astype(F)
    w[w == 0] = 0.5
    if n_targets >= 2:
        w[0] = -0.75
    if n_targets >= 3:
        w[1::3] = 0.0
    return w
