"""Posing on the host: adypt_pose_triangles (csrc/device/pose.hpp) against the numpy restatement (tests/pose_truth.py) bit for bit, against binary64, and
what it refuses.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from adypt_amd import _native as N
from adypt_amd import api
from oracle import oracle_py as O
from tests import pose_truth as P
from tests import refit_truth as T
from tests.helpers import bits

SIZES = (1, 257, 5000)
U = 2.0 ** -24  # the unit roundoff of binary32


def tris_of(n):
    t = T.soup(n)
    t["tc"] = np.random.RandomState(n).uniform(size=t["tc"].shape).astype(np.float32)
    t["matid"] = np.arange(n) % 3 - 1
    return t


def same_triangles(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1))


@pytest.mark.parametrize("n_matrices", [1, 4, 300])
@pytest.mark.parametrize("n", SIZES)
def test_parts_equal_numpy(n, n_matrices):
    tris, mats = tris_of(n), P.matrix_set(n_matrices)
    parts = P.parts_of(n, n_matrices)
    got = api.pose_triangles(tris, mats, parts=parts).view(O.TRI_DT)
    want = P.pose(tris, mats, parts=parts)
    assert same_triangles(got, want)
    assert not np.isnan(got["p"]).any() and not np.isnan(got["n"]).any()
    if n_matrices >= 4 and n >= 4:
        # the zero matrix: len2 == 0, the normal is stored as it came out of the cofactor product — zeros, not NaN
        zero = parts == 3
        assert zero.any() and (got["p"][zero] == 0).all() and (got["n"][zero] == 0).all()
    other = set(tris.dtype.names) - {"p", "n"}
    for f in other:
        assert np.array_equal(bits(got[f]), bits(tris[f])), f


@pytest.mark.parametrize("n_matrices", [1, 4, 300])
@pytest.mark.parametrize("n", SIZES)
def test_skin_equals_numpy(n, n_matrices):
    tris, mats = tris_of(n), P.matrix_set(n_matrices)
    joints, weights = P.skin_of(n, n_matrices)
    got = api.pose_triangles(tris, mats, joints=joints, weights=weights).view(O.TRI_DT)
    want = P.pose(tris, mats, joints=joints, weights=weights)
    assert same_triangles(got, want)
    assert not np.isnan(got["p"]).any() and not np.isnan(got["n"]).any()
    if n >= 257:
        none = (weights == 0).all(axis=-1)
        assert none.any() and (got["p"][none] == 0).all() and (got["n"][none] == 0).all()  # all four weights 0: M = 0


@pytest.mark.parametrize("n", SIZES)
def test_parts_equal_skin_of_one_full_weight(n):
    tris, mats = tris_of(n), P.matrix_set(7)
    parts = P.parts_of(n, 7)
    joints = np.full((n, 3, 4), 65535, dtype=np.uint16)  # out of range in the three slots of weight 0
    joints[..., 0] = parts[:, None]
    weights = np.zeros((n, 3, 4), dtype=np.float32)
    weights[..., 0] = 1.0
    assert same_triangles(api.pose_triangles(tris, mats, parts=parts), api.pose_triangles(tris, mats, joints=joints, weights=weights))
    # ... wherever the one slot stands
    joints2, weights2 = np.roll(joints, 2, axis=-1), np.roll(weights, 2, axis=-1)
    assert same_triangles(api.pose_triangles(tris, mats, parts=parts), api.pose_triangles(tris, mats, joints=joints2, weights=weights2))


def test_positions_against_binary64():
    """|err| <= 9 * 2^-24 * sum_k w_k (sum_j |B_k[r][j]| |x_j| + |B_k[r][3]|): eight roundings on the longest path (w * B, three more slots added, the
    product with the coordinate, three sums), gamma_8 <= 9 u."""
    n, nm = 5000, 300
    tris, mats = tris_of(n), P.matrix_set(nm)
    joints, weights = P.skin_of(n, nm)
    got = api.pose_triangles(tris, mats, joints=joints, weights=weights).view(O.TRI_DT)["p"].astype(np.float64)
    B = mats.astype(np.float64)[np.where(weights == 0, 0, joints).astype(np.int64)]   # [n, 3, 4 (slot), 3, 4]
    w = weights.astype(np.float64)[..., None, None]
    x = np.concatenate([tris["p"].astype(np.float64), np.ones((n, 3, 1))], axis=-1)  # [n, 3, 4]
    exact = ((w * B).sum(axis=2) * x[:, :, None, :]).sum(axis=-1)
    bound = 9 * U * ((w * np.abs(B)).sum(axis=2) * np.abs(x)[:, :, None, :]).sum(axis=-1)
    err = np.abs(got - exact)
    print("positions: largest error over its bound %.3f" % (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all()
    # parts: the same bound with one slot of weight 1
    parts = P.parts_of(n, nm)
    got = api.pose_triangles(tris, mats, parts=parts).view(O.TRI_DT)["p"].astype(np.float64)
    Bp = mats.astype(np.float64)[parts][:, None]                                       # [n, 1, 3, 4]
    exact = (Bp * x[:, :, None, :]).sum(axis=-1)
    bound = 9 * U * (np.abs(Bp) * np.abs(x)[:, :, None, :]).sum(axis=-1)
    assert (np.abs(got - exact) <= bound).all()


def well_conditioned(n, seed=21):
    """n matrices of condition number <= 10: rotation x diag(s) x rotation with s in [1, 10] scaled by a common factor, every fourth mirrored"""
    rs = np.random.RandomState(seed)
    out = []
    for k in range(n):
        s = rs.uniform(1.0, 10.0, size=3) * rs.uniform(0.2, 3.0)
        if k % 4 == 3:
            s[0] = -s[0]
        A = P.rotation(rs.normal(size=3), rs.uniform(0, 360))[:, :3].astype(np.float64) @ np.diag(s) @ P.rotation(rs.normal(size=3), rs.uniform(0, 360))[:, :3].astype(np.float64)
        out.append(np.concatenate([A, rs.normal(size=(3, 1))], axis=1).astype(np.float32))
    m = np.stack(out)
    assert (np.linalg.cond(m[:, :, :3].astype(np.float64)) <= 10.0 * (1 + 1e-5)).all()
    return m


def test_normals_against_binary64():
    """The angle between the posed normal and the binary64 normalised inverse transpose (times the determinant's sign: the cofactor matrix), matrices
    of condition number <= 10.  Largest angle measured on the CPU: 2.617e-07 rad (parts, 5 000 triangles x 3 normals, 300 matrices); asserted at 4 x
    that, 1.047e-06 rad — cancellation in the cofactors has no tidy bound.  The length is held to 1 within 4 u."""
    n, nm = 5000, 300
    tris, mats = tris_of(n), well_conditioned(nm)
    parts = P.parts_of(n, nm)
    got = api.pose_triangles(tris, mats, parts=parts).view(O.TRI_DT)["n"].astype(np.float64)
    A = mats[:, :, :3].astype(np.float64)
    cof = np.linalg.inv(A).transpose(0, 2, 1) * np.linalg.det(A)[:, None, None]
    want = np.einsum("nrc,nvc->nvr", cof[parts], tris["n"].astype(np.float64))
    want /= np.linalg.norm(want, axis=-1, keepdims=True)
    angle = np.arctan2(np.linalg.norm(np.cross(got, want), axis=-1), (got * want).sum(axis=-1))
    print("normals: largest angle %.3e rad" % angle.max())
    assert angle.max() <= 4 * 2.617e-07
    assert np.abs(np.linalg.norm(got, axis=-1) - 1.0).max() <= 4 * U


def refused(tris, mats, parts=None, joints=None, weights=None, n_tris=None, n_matrices=None, out=True):
    """the code of adypt_pose_triangles on raw arrays; the output must stay untouched"""
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    res = np.full_like(t, 0xAB)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    r = N.lib.adypt_pose_triangles(ptr(t), len(t) // 100 if n_tris is None else n_tris, ptr(parts), ptr(joints), ptr(weights), ptr(mats),
                                   len(mats) if n_matrices is None else n_matrices, res.ctypes.data if out else None)
    assert (res == 0xAB).all()
    if r != N.ADYPT_OK:
        assert N.lib.adypt_host_last_error().decode().startswith("adypt_pose_triangles: ")
    return r


def test_refusals():
    n = 10
    tris, mats = tris_of(n), np.ascontiguousarray(P.matrix_set(5).reshape(-1, 12))
    parts = P.parts_of(n, 5)
    joints, weights = (np.ascontiguousarray(a.reshape(-1, 12)) for a in P.skin_of(n, 5))
    assert N.lib.adypt_pose_triangles(tris.ctypes.data, n, parts.ctypes.data, None, None, mats.ctypes.data, 5, np.empty(n * 100, np.uint8).ctypes.data) == N.ADYPT_OK
    E = N.E_INVALID
    # null pointers; both bindings or none
    assert refused(tris, mats, parts, out=False) == E
    assert refused(tris, None, parts, n_matrices=5) == E
    assert refused(tris, mats) == E and refused(tris, mats, joints=joints) == E and refused(tris, mats, weights=weights) == E
    assert refused(tris, mats, parts, joints, weights) == E
    assert refused(tris, mats, parts, n_tris=-1) == E
    # the number of matrices
    assert refused(tris, mats, parts, n_matrices=0) == E and refused(tris, mats, parts, n_matrices=65537) == E
    # indices
    for bad in (-1, 5):
        p = parts.copy()
        p[7] = bad
        assert refused(tris, mats, p) == E
    j = joints.copy()
    slot = np.argwhere(weights != 0)[3]
    j[tuple(slot)] = 5
    assert refused(tris, mats, joints=j, weights=weights) == E
    j = joints.copy()
    j[weights == 0] = 65535  # ... but never in a slot of weight 0
    api.pose_triangles(tris, mats, joints=j, weights=weights)
    # weights
    for bad in (-0.25, np.inf, np.nan):
        w = weights.copy()
        w[4, 5] = bad
        assert refused(tris, mats, joints=joints, weights=w) == E
    # matrices
    for bad in (np.inf, -np.inf, np.nan):
        m = mats.copy()
        m[2, 7] = bad
        assert refused(tris, m, parts) == E and refused(tris, m, joints=joints, weights=weights) == E
    # the binding raises through the Python entry too
    with pytest.raises(N.AdyptError) as e:
        api.pose_triangles(tris, mats, parts=np.full(n, 9, np.int32))
    assert e.value.code == E and "part index" in str(e.value)
    with pytest.raises(N.AdyptError):
        api.pose_triangles(tris, mats)
    assert C.sizeof(N.PoseBinding) == 24
