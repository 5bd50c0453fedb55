"""The truth the tests of the temporal merge by the virtual point use (not a test module): the unfolded length and the virtual point of
csrc/device/guide_chain.hpp and temporal_merge_virtual of csrc/device/temporal.hpp restated in numpy float32 — the operations in the written order, no
fma, a tap that does not count skipped, every refusal written so that a NaN refuses.  The chain itself is tests/specular_truth.py's, walked once more
here with the length beside it; the reprojection is tests/temporal_truth.py's."""
import numpy as np

from oracle import oracle_py as O
from tests import denoise_truth as D
from tests import specular_truth as S
from tests import temporal_truth as TT

F = np.float32
FINITE_MAX = S.FINITE_MAX


class NumpyUnfold:
    """chain_start_length, chain_unfold and chain_virtual_point over arrays."""

    def start_length(self, p0, origin):
        with np.errstate(all="ignore"):
            e = (p0 - np.asarray(origin, np.float32)[None, :]).astype(np.float32)
            return np.sqrt(S.dot(e, e))

    def unfold(self, length, hit, ray_origin):
        with np.errstate(all="ignore"):
            e = (hit - ray_origin).astype(np.float32)
            return length + np.sqrt(S.dot(e, e))

    def virtual_point(self, p0, origin, length):
        """-> (Pv (n, 3), valid (n,))"""
        o = np.asarray(origin, np.float32)[None, :]
        with np.errstate(all="ignore"):
            d0, _ = S.normalize((p0 - o).astype(np.float32))
            pv = (o + d0 * length[:, None]).astype(np.float32)
            valid = (length > 0) & (length <= FINITE_MAX)
        return pv, valid


def chain_guides(osc, P, K, primary=None, ops=None, unfold=None):
    """specular_truth.chain_guides' dict with, beside it, what the unfolding chain leaves at the picture's coordinates: virtual (H, W, 3) and distance
    (H, W) — (Pv, valid ? len : 0) of a pixel whose chain ended on a surface (class >= 2), (the followed P, 0) of every other — and length (H, W): the
    unfolded length itself where a chain ended on a surface, 0 elsewhere."""
    assert 1 <= K <= S.MAX_BOUNCES
    ops, unfold = ops or S.NumpyOps(), unfold or NumpyUnfold()
    g = primary or S.primary_guides(osc, P)
    h, w = g["tri"].shape
    A, Nn, Pp = (g[k].reshape(-1, 3).copy() for k in ("albedo", "normal", "position"))
    P0 = Pp.copy()
    length = np.zeros(h * w, np.float32)
    tri0 = g["tri"].reshape(-1)
    cls = np.where(tri0 != -1, 1, 0).astype(np.int8)
    pix = np.flatnonzero(tri0 != -1)
    bad, illum, kd, ks, ior, dtex = S.materials_of(osc, tri0[pix])
    origin = np.array(list(P.origin), np.float32)
    go, d, T = ops.at_primary(bad, illum, ks, ior, Nn[pix], Pp[pix], origin, K)
    pix, d, T, p = pix[go], d[go], T[go], Pp[pix][go]
    ln = unfold.start_length(p, origin)
    L = np.zeros(len(pix), np.int32)
    counts = dict(rays=0, followed=len(pix), escaped=0, truncated=0)
    for _ in range(K):
        if len(pix) == 0:
            break
        counts["rays"] += len(pix)
        rays = np.zeros((len(pix), 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7] = p, F(P.tmin), d
        hits = O.trace(osc, rays, stack_size=P.stack_size)
        miss = hits["tri_id"] == -1
        e = pix[miss]
        A[e], Nn[e], Pp[e], cls[e] = T[miss], d[miss], F(0), -(L[miss] + 1)
        counts["escaped"] += int(miss.sum())
        keep = ~miss
        pix, d, T, L, hits, ro, ln = pix[keep], d[keep], T[keep], L[keep] + 1, hits[keep], p[keep], ln[keep]
        if len(pix) == 0:
            break
        tri = hits["tri_id"]
        p, n = getattr(ops, "hit_point", S.hit_point)(S.tri_words(osc, tri), hits["u"].copy(), hits["v"].copy())
        ln = unfold.unfold(ln, p, ro)
        bad, illum, kd, ks, ior, dtex = S.materials_of(osc, tri)
        delta = ~bad & (illum >= 3) & (illum <= 7)
        kd = S.textured_kd(osc, tri, hits["u"], hits["v"], kd, np.where(delta, -1, dtex))
        go, albedo, d, T = ops.at_surface(T, d, L, bad, illum, kd, ks, ior, n, K)
        e = pix[~go]
        A[e], Nn[e], Pp[e], cls[e], length[e] = albedo[~go], n[~go], p[~go], 1 + L[~go], ln[~go]
        counts["truncated"] += int((~go & delta).sum())
        pix, d, T, L, p, ln = pix[go], d[go], T[go], L[go], p[go], ln[go]
    assert len(pix) == 0, "a chain outlived its bounces"
    ended = np.flatnonzero(cls >= 2)
    virtual, distance = Pp.copy(), np.zeros(h * w, np.float32)
    pv, valid = unfold.virtual_point(P0[ended], origin, length[ended])
    virtual[ended], distance[ended] = pv, np.where(valid, length[ended], F(0))
    out = dict(albedo=A.reshape(h, w, 3), normal=Nn.reshape(h, w, 3), position=Pp.reshape(h, w, 3), chain=cls.reshape(h, w), hit=(cls != 0).reshape(h, w),
               virtual=virtual.reshape(h, w, 3), distance=distance.reshape(h, w), length=length.reshape(h, w))
    out.update(counts)
    return out


def merge(D0, V0, n, N, P, A, cls, Pv, dist, hist, cap=64.0):
    """temporal_merge_virtual: the merged (D, V, n_out).  cls (H, W) the class of every pixel, (Pv, dist) the XV image; hist None, or what commit() made."""
    h, w = V0.shape
    D0, V0, n = np.asarray(D0, np.float32), np.asarray(V0, np.float32), np.asarray(n, np.float32)
    if hist is None:
        return D0.copy(), V0.copy(), n.copy()
    cap = F(cap)
    cls = np.asarray(cls).astype(np.float32)
    with np.errstate(all="ignore"):
        followed = cls >= F(2.0)
        takes = (cls >= F(1.0)) & (~followed | ((dist > 0) & (dist <= FINITE_MAX)))
        through = np.where(followed[..., None], Pv, P).astype(np.float32)
    ok, fx, fy, far = TT.reproject(hist["cam"], w, h, through)
    with np.errstate(all="ignore"):
        ok = ok & takes & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
        fxs, fys = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        bx, by = np.floor(fxs), np.floor(fys)
        ix, iy = bx.astype(np.int64), by.astype(np.int64)
        ux, uy = fxs - bx, fys - by
        tol = TT.PLANE_TOL * far
        sw, sv, sn = (np.zeros((h, w), np.float32) for _ in range(3))
        sd = np.zeros((h, w, 3), np.float32)
        for ty in (0, 1):
            for tx in (0, 1):
                qx, qy = ix + tx, iy + ty
                counts = ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                Nq, Pq, Aq, Dq, Vq, nq = (hist[k][cy, cx] for k in ("N", "P", "A", "D", "V", "n"))
                counts &= hist["cls"][cy, cx] == cls
                counts &= ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]) >= TT.NORMAL_MIN
                d = Pq - P
                counts &= np.abs((N[..., 0] * d[..., 0] + N[..., 1] * d[..., 1]) + N[..., 2] * d[..., 2]) <= tol
                counts &= (np.abs(Aq - A) <= TT.ALBEDO_TOL).all(-1)
                counts &= (np.abs(Dq) <= FINITE_MAX).all(-1) & (np.abs(Vq) <= FINITE_MAX) & (nq > 0) & (nq <= FINITE_MAX)
                wgt = ((F(1.0) - ux) if tx == 0 else ux) * ((F(1.0) - uy) if ty == 0 else uy)
                sw = np.where(counts, sw + wgt, sw)
                sd = np.where(counts[..., None], sd + wgt[..., None] * Dq, sd)
                sv = np.where(counts, sv + (wgt * wgt) * Vq, sv)
                sn = np.where(counts, sn + wgt * nq, sn)
        take = ok & (sw > TT.MIN_WEIGHT)
        Dh, Vh, hq = sd / sw[..., None], sv / (sw * sw), sn / sw
        nh = np.where(hq < cap, hq, cap).astype(np.float32)
        den = n + nh
        Dm = (n[..., None] * D0 + nh[..., None] * Dh) / den[..., None]
        Vm = ((n * n) * V0 + (nh * nh) * Vh) / (den * den)
        Dm, Vm, no = np.where(take[..., None], Dm, D0), np.where(take, Vm, V0), np.where(take, den, n)
    assert Dm.dtype == np.float32 and Vm.dtype == np.float32 and no.dtype == np.float32
    return Dm, Vm, no


def commit(Dm, Vm, n_out, N, P, A, cls, K, origin, inv_proj, inv_view):
    """what a committing followed call with K bounces leaves: no virtual point, and the mark of its kind"""
    return dict(D=Dm.copy(), V=Vm.copy(), n=n_out.copy(), N=np.array(N, np.float32), P=np.array(P, np.float32), A=np.array(A, np.float32),
                cls=np.asarray(cls).astype(np.float32), kind=("followed", int(K)), cam=TT.camera(origin, inv_proj, inv_view))


def found(hist, K):
    """the history as a followed call with K bounces finds it: only one of its own kind and K"""
    return hist if hist is not None and hist.get("kind") == ("followed", int(K)) else None


def denoise(C, m2, n, g, hist, cam, K, cap=64.0, levels=5, sigma_l=4.0, sigma_z=0.1):
    """One call by the virtual point with the guides g = chain_guides(..., K): (result (H, W, 3), n_out (H, W), the history a commit leaves,
    dict(followed, with_history)).  cam = (origin, inv_proj, inv_view) of this call."""
    C = np.asarray(C, np.float32)
    h, w = C.shape[:2]
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    A, N, P = (np.ascontiguousarray(g[k], np.float32) for k in ("albedo", "normal", "position"))
    cls = g["chain"]
    D0, V0, ka = D.prepare(C, m2, n, A)
    Dm, Vm, n_out = merge(D0, V0, n, N, P, A, cls, g["virtual"], g["distance"], found(hist, K), cap)
    Df, Vf = Dm, Vm
    for i in range(levels):
        Df, Vf = S.level(Df, Vf, N, P, cls, 1 << i, sigma_l, sigma_z)
    with np.errstate(all="ignore"):
        out = Df * ka
    assert out.dtype == np.float32
    counts = dict(followed=int((cls >= 2).sum()), with_history=int(((cls >= 2) & (n_out > n)).sum()))
    return out, n_out, commit(Dm, Vm, n_out, N, P, A, cls, K, *cam), counts
