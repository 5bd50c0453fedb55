"""The truth the rectification tests use (not a test module): csrc/device/rectify.hpp, and the rectified form of temporal_merge_through of
csrc/device/temporal.hpp, restated in numpy float32 on top of tests/temporal_truth.py — the operations in the written order, no fma, a tap that does
not count skipped (an accumulator keeps its word), every refusal written so that a NaN refuses."""
import numpy as np

from tests import denoise_truth as D
from tests import temporal_motion_truth as TM
from tests import temporal_truth as TT

F = np.float32
MIN_TAPS, DEFAULT_RADIUS, DEFAULT_GAMMA = F(4), 3, 1.0


def window(D0, V0, N, P, A, hit, origin, radius=DEFAULT_RADIUS):
    """rectify_window of every pixel of the current call's images: R0 = (mu.rgb, k), R1 = (g.rgb, 0), both (H, W, 4) float32."""
    D0, V0, N, P, A = (np.asarray(v, np.float32) for v in (D0, V0, N, P, A))
    hit = np.asarray(hit).astype(bool)
    h, w = V0.shape
    o = np.asarray(origin, np.float32).reshape(3)
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        e = [P[..., i] - o[i] for i in range(3)]
        tol = TT.PLANE_TOL * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        k, v = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        s, t = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                qx, qy = xx + dx, yy + dy
                counts = hit & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                Nq, Pq, Aq, Dq, Vq = (a[cy, cx] for a in (N, P, A, D0, V0))
                counts &= hit[cy, cx]
                counts &= ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]) >= TT.NORMAL_MIN
                d = Pq - P
                counts &= np.abs((N[..., 0] * d[..., 0] + N[..., 1] * d[..., 1]) + N[..., 2] * d[..., 2]) <= tol
                counts &= (np.abs(Aq - A) <= TT.ALBEDO_TOL).all(-1)
                counts &= (np.abs(Dq) <= TT.FINITE_MAX).all(-1) & (np.abs(Vq) <= TT.FINITE_MAX)
                k = np.where(counts, k + F(1.0), k)
                s = np.where(counts[..., None], s + Dq, s)
                t = np.where(counts[..., None], t + Dq * Dq, t)
                v = np.where(counts, v + Vq, v)
        have = k > 0
        kk = k[..., None]
        mu = s / kk
        var = t / kk - mu * mu
        var = np.where(var > 0, var, F(0))
        ex = var - (v / k)[..., None]
        ex = np.where(ex > 0, ex, F(0))
        g = ex + var / kk
        mu, g = np.where(have[..., None], mu, F(0)), np.where(have[..., None], g, F(0))
    R0 = np.concatenate([mu, k[..., None]], -1).astype(np.float32, copy=False)
    R1 = np.concatenate([g, np.zeros((h, w, 1), np.float32)], -1).astype(np.float32, copy=False)
    assert mu.dtype == np.float32 and g.dtype == np.float32 and k.dtype == np.float32
    return np.ascontiguousarray(R0), np.ascontiguousarray(R1)


def history_taps(N, P, A, hit, hist, w, h):
    """The four bilinear taps of temporal_merge_through for the surface (N, P) given: (take, Dh, Vh, hq) — whether the pixel found history, and the
    history's colour, variance and length there (temporal_truth.merge's loop, stopped before the cap and the blend)."""
    ok, fx, fy, dist = TT.reproject(hist["cam"], w, h, P)
    with np.errstate(all="ignore"):
        ok = ok & hit & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
        fxs, fys = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        bx, by = np.floor(fxs), np.floor(fys)
        ix, iy = bx.astype(np.int64), by.astype(np.int64)
        ux, uy = fxs - bx, fys - by
        tol = TT.PLANE_TOL * dist
        sw, sv, sn = (np.zeros((h, w), np.float32) for _ in range(3))
        sd = np.zeros((h, w, 3), np.float32)
        for ty in (0, 1):
            for tx in (0, 1):
                qx, qy = ix + tx, iy + ty
                counts = ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                Nq, Pq, Aq, Dq, Vq, nq = (hist[k][cy, cx] for k in ("N", "P", "A", "D", "V", "n"))
                counts &= hist["hit"][cy, cx].astype(bool)
                counts &= ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]) >= TT.NORMAL_MIN
                d = Pq - P
                counts &= np.abs((N[..., 0] * d[..., 0] + N[..., 1] * d[..., 1]) + N[..., 2] * d[..., 2]) <= tol
                counts &= (np.abs(Aq - A) <= TT.ALBEDO_TOL).all(-1)
                counts &= (np.abs(Dq) <= TT.FINITE_MAX).all(-1) & (np.abs(Vq) <= TT.FINITE_MAX) & (nq > 0) & (nq <= TT.FINITE_MAX)
                wgt = ((F(1.0) - ux) if tx == 0 else ux) * ((F(1.0) - uy) if ty == 0 else uy)
                sw = np.where(counts, sw + wgt, sw)
                sd = np.where(counts[..., None], sd + wgt[..., None] * Dq, sd)
                sv = np.where(counts, sv + (wgt * wgt) * Vq, sv)
                sn = np.where(counts, sn + wgt * nq, sn)
        take = ok & (sw > TT.MIN_WEIGHT)
        return take, sd / sw[..., None], sv / (sw * sw), sn / sw


def merge(D0, V0, n, N, P, A, hit, hist, R0, R1, gamma=DEFAULT_GAMMA, cap=64.0, through=None):
    """The rectified merge of every pixel: (Dm, Vm, n_out, kept).  through: None, or (N_prev, P_prev, valid) of the motion form, which the history is
    reprojected and tested through while the window statistics stay the current pose's."""
    D0, V0, n = np.asarray(D0, np.float32), np.asarray(V0, np.float32), np.asarray(n, np.float32)
    h, w = V0.shape
    if hist is None:
        return D0.copy(), V0.copy(), n.copy(), np.ones((h, w), np.float32)
    cap, gamma = F(cap), F(gamma)
    hit = np.asarray(hit).astype(bool)
    if through is not None:
        N, P, hit = np.asarray(through[0], np.float32), np.asarray(through[1], np.float32), hit & np.asarray(through[2]).astype(bool)
    take, Dh, Vh, hq = history_taps(np.asarray(N, np.float32), np.asarray(P, np.float32), np.asarray(A, np.float32), hit, hist, w, h)
    with np.errstate(all="ignore"):
        nh = np.where(hq < cap, hq, cap).astype(np.float32)
        applies = take & (R0[..., 3] >= MIN_TAPS)
        mu, lim = R0[..., :3], gamma * np.sqrt(R1[..., :3])
        d = np.abs(Dh - mu)
        keeps = d <= lim
        Dc = np.where(keeps, Dh, np.where(Dh < mu, mu - lim, mu + lim))
        fc = np.where(keeps, F(1.0), lim / d)
        f = fc[..., 0]
        f = np.where(fc[..., 1] < f, fc[..., 1], f)
        f = np.where(fc[..., 2] < f, fc[..., 2], f)
        f = np.where((fc >= 0).all(-1), f, F(0))
        kept = np.where(applies, f, F(1.0)).astype(np.float32)
        Dh = np.where(applies[..., None], Dc, Dh)
        nh = np.where(applies, nh * f, nh)
        take = take & ~(applies & ~(nh > 0))
        den = n + nh
        Dm = (n[..., None] * D0 + nh[..., None] * Dh) / den[..., None]
        Vm = ((n * n) * V0 + (nh * nh) * Vh) / (den * den)
        Dm, Vm, no = np.where(take[..., None], Dm, D0), np.where(take, Vm, V0), np.where(take, den, n)
    assert Dm.dtype == np.float32 and Vm.dtype == np.float32 and no.dtype == np.float32 and kept.dtype == np.float32
    return Dm, Vm, no, kept


def denoise(C, m2, n, A, N, P, hit, hist, cam, radius=DEFAULT_RADIUS, gamma=DEFAULT_GAMMA, cap=64.0, levels=5, sigma_l=4.0, sigma_z=0.1, motion=None):
    """One rectified temporal call: (result (H, W, 3), n_out (H, W), the history a commit leaves, dict(kept, R0, R1, D, V)).  cam = (origin, inv_proj,
    inv_view) of this call; motion: None, or (tri, uv, cur) of a call that follows moved geometry (temporal_motion_truth.denoise's arguments)."""
    C = np.asarray(C, np.float32)
    h, w = C.shape[:2]
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    A, N, P = (np.ascontiguousarray(v, np.float32) for v in (A, N, P))
    hit = np.asarray(hit).astype(bool)
    D0, V0, ka = D.prepare(C, m2, n, A)
    R0, R1 = window(D0, V0, N, P, A, hit, cam[0], radius)
    through = None
    if motion is not None:
        tri, uv, cur = motion
        Pp, _, Np, valid = TM.previous_point(None if hist is None else hist.get("tris"), cur, tri, uv, N, P)
        through = (Np, Pp, valid)
    Dm, Vm, n_out, kept = merge(D0, V0, n, N, P, A, hit, hist, R0, R1, gamma, cap, through)
    Df, Vf = Dm, Vm
    for i in range(levels):
        Df, Vf = D.level(Df, Vf, N, P, hit, 1 << i, sigma_l, sigma_z)
    with np.errstate(all="ignore"):
        out = Df * ka
    assert out.dtype == np.float32
    new = TT.commit(Dm, Vm, n_out, N, P, A, hit, *cam)
    if motion is not None:
        new["tris"] = np.array(motion[2], np.float32).reshape(-1, TM.TRI_WORDS).copy()
    return out, n_out, new, dict(kept=kept, R0=R0, R1=R1, D=Dm, V=Vm)
