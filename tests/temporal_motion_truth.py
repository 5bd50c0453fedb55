"""The truth the motion tests of the temporal merge use (not a test module): temporal_previous_point and temporal_merge_motion of
csrc/device/temporal.hpp restated in numpy float32 on top of tests/temporal_truth.py — the operations in the written order, no fma, every refusal
written so that a NaN refuses.  A history is what temporal_truth.commit makes plus "tris": words 0..17 of every triangle record at that commit
((n, 18) float32), or None where the commit was not a motion call."""
import numpy as np

from tests import denoise_truth as D
from tests import temporal_truth as TT

F = np.float32
TRI_WORDS = 18


def tri_words(p, n):
    """(count, 18) float32: p0 p1 p2 n0 n1 n2 of every triangle, from positions and normals of shape (count, 3, 3) (or (count, 9))."""
    p, n = np.asarray(p, np.float32).reshape(-1, 9), np.asarray(n, np.float32).reshape(-1, 9)
    return np.ascontiguousarray(np.concatenate([p, n], axis=1))


def previous_point(prev, cur, tri, uv, N, P):
    """temporal_previous_point of every pixel: (P_prev (H, W, 3), moved (H, W) bool, N_prev (H, W, 3), valid (H, W) bool).  prev: the snapshot
    ((n_snapshot, 18) float32) or None; cur: the records now; tri: the hit's triangle index (any int32: -1 is sky, an index outside the snapshot a
    stranger — neither is used as an index); uv (H, W, 2)."""
    N, P = np.asarray(N, np.float32), np.asarray(P, np.float32)
    tri = np.asarray(tri).astype(np.int64)
    h, w = tri.shape
    Pp, Np = P.copy(), N.copy()
    moved, valid = np.zeros((h, w), bool), np.ones((h, w), bool)
    if prev is None or len(prev) == 0 or len(cur) == 0:
        return Pp, moved, Np, valid
    prev, cur = np.asarray(prev, np.float32).reshape(-1, TRI_WORDS), np.asarray(cur, np.float32).reshape(-1, TRI_WORDS)
    known = (tri >= 0) & (tri < len(prev)) & (tri < len(cur))
    t = np.where(known, tri, 0)
    a, b = prev[t], cur[t]  # (H, W, 18)
    moved = known & (a.view(np.uint32) != b.view(np.uint32)).any(-1)
    u, v = np.asarray(uv, np.float32)[..., 0], np.asarray(uv, np.float32)[..., 1]
    with np.errstate(all="ignore"):
        wgt = (F(1.0) - u) - v
        pp = np.stack([(a[..., k] * u + a[..., 3 + k] * v) + a[..., 6 + k] * wgt for k in range(3)], -1)
        nn = np.stack([(a[..., 9 + k] * u + a[..., 12 + k] * v) + a[..., 15 + k] * wgt for k in range(3)], -1)
        len2 = (nn[..., 0] * nn[..., 0] + nn[..., 1] * nn[..., 1]) + nn[..., 2] * nn[..., 2]
        good = (len2 > 0) & (len2 <= TT.FINITE_MAX)
        nn = nn / np.sqrt(len2)[..., None]
    assert pp.dtype == np.float32 and nn.dtype == np.float32
    Pp = np.where(moved[..., None], pp, Pp)
    Np = np.where(moved[..., None], np.where(good[..., None], nn, F(0)), Np)
    valid = ~moved | good
    return Pp, moved, Np, valid


def merge(D0, V0, n, N, P, A, hit, hist, tri, uv, cur, cap=64.0):
    """temporal_merge_motion of every pixel: (Dm, Vm, n_out, motion) with motion = dict(previous_position, moved, previous_normal, valid)."""
    prev = None if hist is None else hist.get("tris")
    Pp, moved, Np, valid = previous_point(prev, cur, tri, uv, N, P)
    motion = dict(previous_position=Pp, moved=moved, previous_normal=Np, valid=valid)
    # (temporal_truth.merge reads N and P for the reprojection and the taps' normal and plane tests only: given the previous ones it is the motion form)
    Dm, Vm, no = TT.merge(D0, V0, n, Np, Pp, A, np.asarray(hit).astype(bool) & valid, hist, cap)
    return Dm, Vm, no, motion


def denoise(C, m2, n, A, N, P, hit, hist, cam, tri, uv, cur, cap=64.0, levels=5, sigma_l=4.0, sigma_z=0.1):
    """One motion call: (result, n_out, the history a commit leaves — with the snapshot `cur` —, motion)."""
    C = np.asarray(C, np.float32)
    h, w = C.shape[:2]
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    A, N, P = (np.ascontiguousarray(v, np.float32) for v in (A, N, P))
    hit = np.asarray(hit).astype(bool)
    D0, V0, ka = D.prepare(C, m2, n, A)
    Dm, Vm, n_out, motion = merge(D0, V0, n, N, P, A, hit, hist, tri, uv, cur, cap)
    Df, Vf = Dm, Vm
    for i in range(levels):
        Df, Vf = D.level(Df, Vf, N, P, hit, 1 << i, sigma_l, sigma_z)
    with np.errstate(all="ignore"):
        out = Df * ka
    assert out.dtype == np.float32
    new = TT.commit(Dm, Vm, n_out, N, P, A, hit, *cam)
    new["tris"] = np.array(cur, np.float32).reshape(-1, TRI_WORDS).copy()
    return out, n_out, new, motion
