"""Morph targets on the host: adypt_pose_triangles_morph (csrc/device/pose.hpp) against the numpy restatement (tests/morph_truth.py) bit for bit, the
order of a triangle's entries, zero weights, against binary64, adypt_morph_diff, and what is refused.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from adypt_amd import _native as N
from adypt_amd import api
from oracle import oracle_py as O
from tests import morph_truth as M
from tests import pose_truth as P
from tests.helpers import bits
from tests.test_pose_definition import SIZES, U, same_triangles, tris_of


def binding_of(kind, n, nm):
    if kind == "parts":
        return {"parts": P.parts_of(n, nm)}
    j, w = P.skin_of(n, nm)
    return {"joints": j, "weights": w}


def one_part(n):
    return {"parts": np.zeros(n, np.int32)}


IDENTITY = P.identity()[None]


@pytest.mark.parametrize("kind", ["parts", "skin"])
@pytest.mark.parametrize("n_targets", [1, 3, 300])
@pytest.mark.parametrize("n", SIZES)
def test_morph_equals_numpy(n, n_targets, kind):
    tris, mats, binding = tris_of(n), P.matrix_set(5), binding_of(kind, n, 5)
    entries, w = M.entries_of(n, n_targets), M.weights_of(n_targets)
    count = np.bincount(entries[0], minlength=n)
    assert count[n - 1] > 0 and count.max() == n_targets
    if n >= 5:
        assert count[0] == 0 and count[1] == 1                       # a triangle with none, one with one, one with every target
    got = api.pose_triangles(tris, mats, morph=entries, morph_weights=w, **binding)
    want = M.pose(tris, mats, entries, w, **binding)
    assert same_triangles(got, want)
    assert not same_triangles(got, api.pose_triangles(tris, mats, **binding))              # the layer shows
    for f in set(tris.dtype.names) - {"p", "n"}:
        assert np.array_equal(bits(got.view(O.TRI_DT)[f]), bits(tris[f])), f
    # the order the entries are given in is not the order they are taken in
    shuffle = np.random.RandomState(n).permutation(len(entries[0]))
    again = api.pose_triangles(tris, mats, morph=tuple(a[shuffle] for a in entries), morph_weights=w, **binding)
    assert same_triangles(again, got)
    # the [n, 2, 3, 3] form of the deltas
    assert same_triangles(api.pose_triangles(tris, mats, morph=(entries[0], entries[1], entries[2].reshape(-1, 2, 3, 3)), morph_weights=w, **binding), got)


def test_entries_are_taken_in_ascending_target_index():
    """(0 + 1e8) - 1e8 + 1 = 1 in binary32, (0 + 1) + 1e8 - 1e8 = 0: the order shows, and the one of the definition is by target index."""
    tris = tris_of(3)
    tris["p"][1, 0, 0] = 0.0
    d = np.zeros((3, 18), np.float32)
    d[:, 0] = (1e8, -1e8, 1.0)                                                             # targets 0, 1, 2 on word 0 of triangle 1
    tri, w = np.ones(3, np.int32), np.ones(3, np.float32)
    results = []
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0], [2, 1, 0]):
        o = np.array(order)
        got = api.pose_triangles(tris, IDENTITY, morph=(tri[o], o.astype(np.int32), d[o]), morph_weights=w, **one_part(3)).view(O.TRI_DT)
        results.append(got["p"][1, 0, 0])
    assert results == [1.0] * 4
    # the other order of the same three deltas — 1 first — gives another number
    swapped = api.pose_triangles(tris, IDENTITY, morph=(tri, np.array([1, 2, 0], np.int32), d), morph_weights=w, **one_part(3)).view(O.TRI_DT)
    assert swapped["p"][1, 0, 0] == 0.0


@pytest.mark.parametrize("kind", ["parts", "skin"])
def test_zero_weights_leave_no_trace(kind):
    n, nt = 257, 3
    tris, mats, binding = tris_of(n), P.matrix_set(5), binding_of(kind, n, 5)
    tris["p"][3, 1, 2] = -0.0
    tris["n"][4, 0, 0] = -0.0
    entries = M.entries_of(n, nt)
    plain = api.pose_triangles(tris, mats, **binding)
    assert same_triangles(api.pose_triangles(tris, mats, morph=entries, morph_weights=np.zeros(nt, np.float32), **binding), plain)
    assert same_triangles(api.pose_triangles(tris, mats, morph=entries, morph_weights=np.array([0.0, -0.0, 0.0], np.float32), **binding), plain)
    # (the matrix stage turns a -0.0 into +0.0 by its sums, with or without a layer; the morph stage alone, in the restatement, keeps the sign)
    stage = M.morph(tris, *entries, np.zeros(nt, np.float32))
    assert same_triangles(stage, tris) and np.signbit(stage["p"][3, 1, 2]) and np.signbit(stage["n"][4, 0, 0])
    # a target of weight 0 whose deltas are huge: never read, never multiplied (0 * 3e38 would be harmless, 3e38 + 3e38 not)
    w = M.weights_of(nt)
    assert w[1] == 0 and w[0] != 0 and w[2] != 0
    huge = entries[2].copy()
    huge[entries[1] == 1] = 3e38
    assert (entries[1] == 1).any()
    got = api.pose_triangles(tris, mats, morph=(entries[0], entries[1], huge), morph_weights=w, **binding)
    assert same_triangles(got, api.pose_triangles(tris, mats, morph=entries, morph_weights=w, **binding))
    assert np.isfinite(got.view(O.TRI_DT)["p"]).all()


def test_negative_weights_are_accepted():
    n, nt = 50, 3
    tris, entries = tris_of(n), M.entries_of(n, nt)
    w = np.array([-1.0, -0.5, -2.0], np.float32)
    got = api.pose_triangles(tris, IDENTITY, morph=entries, morph_weights=w, **one_part(n))
    assert same_triangles(got, M.pose(tris, IDENTITY, entries, w, **one_part(n)))
    assert not same_triangles(got, api.pose_triangles(tris, IDENTITY, morph=entries, morph_weights=-w, **one_part(n)))


def test_positions_against_binary64():
    """The morph stage alone: one part, the exact identity, so p' = ((1 * x + 0 * y) + 0 * z) + 0 = x without a rounding.  A word with K active entries
    is acc_K, acc_k = fl(acc_(k-1) + fl(w_k d_k)): K products and K sums.  The rest pose's word goes through the K sums, entry k through its product and
    the sums k..K; the longest path is entry 1's, K + 1 roundings, so |acc_K - (x + sum_k w_k d_k)| <= gamma_(K+1) (|x| + sum_k |w_k d_k|) with
    gamma_m = m u / (1 - m u), u = 2^-24.  The binary64 sum it is held against is itself off by at most K 2^-53 of the same magnitude, which is added."""
    n, nt = 5000, 300
    tris, entries, w = tris_of(n), M.entries_of(n, nt), M.weights_of(nt)
    got = api.pose_triangles(tris, IDENTITY, morph=entries, morph_weights=w, **one_part(n)).view(O.TRI_DT)["p"].astype(np.float64).reshape(n, 9)
    tri, tgt, d = entries
    x = tris["p"].astype(np.float64).reshape(n, 9)
    term = w.astype(np.float64)[tgt][:, None] * d.astype(np.float64)[:, :9]                # exact: a product of two binary32 numbers
    exact, mag = x.copy(), np.abs(x)
    np.add.at(exact, tri, term)
    np.add.at(mag, tri, np.abs(term))
    K = np.bincount(tri[w[tgt] != 0], minlength=n).astype(np.float64)[:, None]
    assert K.max() == (w != 0).sum() and K.min() == 0
    gamma = (K + 1) * U / (1 - (K + 1) * U)
    bound = np.where(K > 0, gamma * mag + K * 2.0 ** -53 * mag, 0.0)
    err = np.abs(got - exact)
    print("morphed positions: largest error over its bound %.3f" % (err[K[:, 0] > 0] / bound[K[:, 0] > 0]).max())
    assert (err <= bound).all()


def test_morph_diff_lists_the_triangles_that_differ_in_any_bit():
    n = 300
    rest = tris_of(n)
    rest["p"][7, 2, 1] = 0.0
    target = rest.copy()
    moved = np.array([3, 7, 8, 120, 299])
    target["p"][3] += np.float32(0.25)
    target["p"][7, 2, 1] = -0.0                                                            # another bit pattern of the same number: listed, delta 0
    target["n"][8, 1] = (0.0, 1.0, 0.0)
    target["p"][120, 0, 0] += np.float32(1e-3)
    target["n"][299, 2, 2] -= np.float32(0.5)
    target["tc"][50] += np.float32(0.5)                                                    # texture coordinates and material ids are not morphed
    target["matid"][51] = 7
    tri, d = api.morph_diff(rest, target)
    assert tri.dtype == np.int32 and d.dtype == np.float32 and d.shape == (5, 18)
    assert np.array_equal(tri, moved)
    a = np.concatenate([rest["p"].reshape(n, 9), rest["n"].reshape(n, 9)], axis=1)
    b = np.concatenate([target["p"].reshape(n, 9), target["n"].reshape(n, 9)], axis=1)
    assert np.array_equal(bits(d), bits((b[moved] - a[moved]).astype(np.float32)))
    assert (d[1] == 0).all()
    # the size alone; nothing differs; what is refused
    ptr = lambda x: np.ascontiguousarray(x).view(np.uint8).ctypes.data  # noqa: E731
    assert N.lib.adypt_morph_diff(ptr(rest), ptr(target), n, None, None) == 5
    none = api.morph_diff(rest, rest)
    assert len(none[0]) == 0 and none[1].shape == (0, 18)
    assert N.lib.adypt_morph_diff(None, ptr(target), n, None, None) == N.E_INVALID
    assert N.lib.adypt_morph_diff(ptr(rest), None, n, None, None) == N.E_INVALID
    assert N.lib.adypt_morph_diff(ptr(rest), ptr(target), -1, None, None) == N.E_INVALID
    assert N.lib.adypt_host_last_error().decode().startswith("adypt_morph_diff: ")
    with pytest.raises(ValueError):
        api.morph_diff(rest, target[:-1])
    # weight 1 gives rest + (target - rest): the target up to the rounding of the difference, u (|target| + |rest|), and that of the sum, u |target|
    got = api.pose_triangles(rest, IDENTITY, morph=(tri, np.zeros(5, np.int32), d), morph_weights=[1.0], **one_part(n)).view(O.TRI_DT)
    assert np.abs(got["p"].astype(np.float64) - target["p"].astype(np.float64)).max() <= 4 * U * max(np.abs(target["p"]).max(), np.abs(rest["p"]).max())


def refused(tris, tri, tgt, d, w, n_entries=None, n_targets=None):
    """the code of adypt_pose_triangles_morph on raw arrays, one part under the identity; the output must stay untouched"""
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    n = len(t) // 100
    parts, mats = np.zeros(n, np.int32), np.ascontiguousarray(IDENTITY.reshape(-1, 12))
    res = np.full_like(t, 0xAB)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    r = N.lib.adypt_pose_triangles_morph(t.ctypes.data, n, parts.ctypes.data, None, None, mats.ctypes.data, 1, ptr(tri), ptr(tgt), ptr(d),
                                         len(tri) if n_entries is None else n_entries, ptr(w), len(w) if n_targets is None else n_targets, res.ctypes.data)
    if r != N.ADYPT_OK:
        assert (res == 0xAB).all()
        assert N.lib.adypt_host_last_error().decode().startswith("adypt_pose_triangles_morph: ")
    return r


def test_refusals():
    n, nt = 10, 3
    tris = tris_of(n)
    tri, tgt, d = M.entries_of(n, nt)
    w = M.weights_of(nt)
    ne, E = len(tri), N.E_INVALID
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    out = np.empty_like(t)
    parts, mats = np.zeros(n, np.int32), np.ascontiguousarray(IDENTITY.reshape(-1, 12))
    assert N.lib.adypt_pose_triangles_morph(t.ctypes.data, n, parts.ctypes.data, None, None, mats.ctypes.data, 1, tri.ctypes.data, tgt.ctypes.data, d.ctypes.data, ne, w.ctypes.data,
                                            nt, out.ctypes.data) == N.ADYPT_OK
    # a null array
    assert refused(tris, None, tgt, d, w, n_entries=ne) == E
    assert refused(tris, tri, None, d, w) == E
    assert refused(tris, tri, tgt, None, w) == E
    assert refused(tris, tri, tgt, d, None, n_targets=nt) == E
    assert N.lib.adypt_pose_triangles_morph(t.ctypes.data, n, parts.ctypes.data, None, None, mats.ctypes.data, 1, tri.ctypes.data, tgt.ctypes.data, d.ctypes.data, ne, w.ctypes.data,
                                            nt, None) == E
    # the counts
    for bad in (0, -1, 2 ** 31):
        assert refused(tris, tri, tgt, d, w, n_entries=bad) == E
    big = np.zeros(65537, np.float32)
    assert refused(tris, tri, tgt, d, w, n_targets=0) == E and refused(tris, tri, tgt, d, big) == E
    assert refused(tris, tri, tgt, d, big[:65536]) == N.ADYPT_OK
    # the indices
    for bad in (-1, n):
        a = tri.copy()
        a[2] = bad
        assert refused(tris, a, tgt, d, w) == E
    for bad in (-1, nt):
        a = tgt.copy()
        a[ne - 1] = bad
        assert refused(tris, tri, a, d, w) == E
    assert refused(tris, tri, tgt, d, w[:-1]) == E                                         # fewer weights than the entries' targets
    # the deltas
    for bad in (np.inf, -np.inf, np.nan):
        a = d.copy()
        a[ne // 2, 17] = bad
        assert refused(tris, tri, tgt, a, w) == E
    # two entries of one (triangle, target), wherever they stand
    assert refused(tris, np.append(tri, tri[0]), np.append(tgt, tgt[0]), np.concatenate([d, d[:1]]), w) == E
    # the weights
    for bad in (np.inf, -np.inf, np.nan):
        a = w.copy()
        a[1] = bad
        assert refused(tris, tri, tgt, d, a) == E
    # ... and through the Python entry
    with pytest.raises(N.AdyptError) as e:
        api.pose_triangles(tris, IDENTITY, morph=(tri, tgt, d), morph_weights=[1.0, np.nan, 0.0], **one_part(n))
    assert e.value.code == E and "morph weight" in str(e.value)
    with pytest.raises(ValueError):
        api.pose_triangles(tris, IDENTITY, morph=(tri, tgt, d), **one_part(n))
    with pytest.raises(ValueError):
        api.pose_triangles(tris, IDENTITY, morph=(tri, tgt[:-1], d), morph_weights=w, **one_part(n))
    assert C.sizeof(N.MorphBinding) == 32 and C.sizeof(N.PoseBinding) == 24
