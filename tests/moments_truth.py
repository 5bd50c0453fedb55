"""The truth the moments tests use (not a test module): csrc/device/moments.hpp, and the moments form of temporal_merge_through of
csrc/device/temporal.hpp, restated in numpy float32 on top of tests/temporal_truth.py — the operations in the written order, no fma, a tap that does
not count skipped (an accumulator keeps its word), every refusal written so that a NaN refuses.  A history is what temporal_truth.commit makes, its
"V" holding S, marked moments=True: a call finds only a history of its own kind (history_for)."""
import numpy as np

from tests import denoise_truth as D
from tests import temporal_motion_truth as TM
from tests import temporal_truth as TT

F = np.float32
MIN_LENGTH, RADIUS, MIN_TAPS = F(4), 3, F(4)


def history_for(hist, moments):
    """What a call of the kind given finds in `hist`: the history itself, or None where another kind of call wrote it."""
    if hist is None or bool(hist.get("moments", False)) != bool(moments):
        return None
    return hist


def prepare(C, m2, n, A):
    """moments_prepare: (D0, S0, A + 0.01)."""
    C, m2, n, A = (np.asarray(v, np.float32) for v in (C, m2, n, A))
    with np.errstate(all="ignore"):
        la = D.lum(A) + F(0.01)
        ka = A + F(0.01)
        D0 = C / ka
        Y = D.lum(D0)
        S0 = Y * Y + (m2 / n) / (la * la)
    assert D0.dtype == np.float32 and S0.dtype == np.float32
    return D0, S0, ka


def merge(D0, S0, n, N, P, A, hit, hist, cap=64.0, through=None, square_tap_weight=False):
    """temporal_merge_through<true> of every pixel: (Dm, S, n_out).  through: None, or (N_prev, P_prev, valid) of the motion form.
    square_tap_weight=True: a tap's S taken with w * w instead of w (not part of the definition: what an edge input must tell from it)."""
    D0, S0, n = np.asarray(D0, np.float32), np.asarray(S0, np.float32), np.asarray(n, np.float32)
    h, w = S0.shape
    if hist is None:
        return D0.copy(), S0.copy(), n.copy()
    cap = F(cap)
    hit = np.asarray(hit).astype(bool)
    N, P, A = (np.asarray(v, np.float32) for v in (N, P, A))
    if through is not None:
        N, P, hit = np.asarray(through[0], np.float32), np.asarray(through[1], np.float32), hit & np.asarray(through[2]).astype(bool)
    ok, fx, fy, dist = TT.reproject(hist["cam"], w, h, P)
    with np.errstate(all="ignore"):
        ok = ok & hit & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
        fxs, fys = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        bx, by = np.floor(fxs), np.floor(fys)
        ix, iy = bx.astype(np.int64), by.astype(np.int64)
        ux, uy = fxs - bx, fys - by
        tol = TT.PLANE_TOL * dist
        sw, ss, sn = (np.zeros((h, w), np.float32) for _ in range(3))
        sd = np.zeros((h, w, 3), np.float32)
        for ty in (0, 1):
            for tx in (0, 1):
                qx, qy = ix + tx, iy + ty
                counts = ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                Nq, Pq, Aq, Dq, Sq, nq = (hist[k][cy, cx] for k in ("N", "P", "A", "D", "V", "n"))
                counts &= hist["hit"][cy, cx].astype(bool)
                counts &= ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]) >= TT.NORMAL_MIN
                d = Pq - P
                counts &= np.abs((N[..., 0] * d[..., 0] + N[..., 1] * d[..., 1]) + N[..., 2] * d[..., 2]) <= tol
                counts &= (np.abs(Aq - A) <= TT.ALBEDO_TOL).all(-1)
                counts &= (np.abs(Dq) <= TT.FINITE_MAX).all(-1) & (np.abs(Sq) <= TT.FINITE_MAX) & (nq > 0) & (nq <= TT.FINITE_MAX)
                wgt = ((F(1.0) - ux) if tx == 0 else ux) * ((F(1.0) - uy) if ty == 0 else uy)
                sw = np.where(counts, sw + wgt, sw)
                sd = np.where(counts[..., None], sd + wgt[..., None] * Dq, sd)
                ss = np.where(counts, ss + (wgt * wgt if square_tap_weight else wgt) * Sq, ss)
                sn = np.where(counts, sn + wgt * nq, sn)
        take = ok & (sw > TT.MIN_WEIGHT)
        Dh, Sh, hq = sd / sw[..., None], ss / sw, sn / sw
        nh = np.where(hq < cap, hq, cap).astype(np.float32)
        den = n + nh
        Dm = (n[..., None] * D0 + nh[..., None] * Dh) / den[..., None]
        Sm = (n * S0 + nh * Sh) / den
        Dm, Sm, no = np.where(take[..., None], Dm, D0), np.where(take, Sm, S0), np.where(take, den, n)
    assert Dm.dtype == np.float32 and Sm.dtype == np.float32 and no.dtype == np.float32
    return Dm, Sm, no


def variance(Dm, S, n_out, N, P, A, hit, origin, window=True):
    """moments_variance of every pixel of the merged images: (V, spatial, k) — the variance the first level sees, which pixels took the window estimate,
    and the counting taps of every pixel that asked its window (0 elsewhere).  window=False: no pixel asks (what the issue's table calls 'without the
    spatial window'; not part of the definition)."""
    Dm, S, n_out, N, P, A = (np.asarray(v, np.float32) for v in (Dm, S, n_out, N, P, A))
    hit = np.asarray(hit).astype(bool)
    h, w = S.shape
    o = np.asarray(origin, np.float32).reshape(3)
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        Y = D.lum(Dm)
        own = S - Y * Y
        own = np.where(own > 0, own, F(0))
        asks = hit & (n_out < MIN_LENGTH) & bool(window)
        e = [P[..., i] - o[i] for i in range(3)]
        tol = TT.PLANE_TOL * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        k, s1, s2 = (np.zeros((h, w), np.float32) for _ in range(3))
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                qx, qy = xx + dx, yy + dy
                counts = asks & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                Nq, Pq, Aq, Yq, Sq = (a[cy, cx] for a in (N, P, A, Y, S))
                counts &= hit[cy, cx]
                counts &= ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]) >= TT.NORMAL_MIN
                d = Pq - P
                counts &= np.abs((N[..., 0] * d[..., 0] + N[..., 1] * d[..., 1]) + N[..., 2] * d[..., 2]) <= tol
                counts &= (np.abs(Aq - A) <= TT.ALBEDO_TOL).all(-1)
                counts &= (np.abs(Yq) <= TT.FINITE_MAX) & (np.abs(Sq) <= TT.FINITE_MAX)
                k = np.where(counts, k + F(1.0), k)
                s1 = np.where(counts, s1 + Yq, s1)
                s2 = np.where(counts, s2 + Sq, s2)
        spatial = asks & (k >= MIN_TAPS)
        mu1, mu2 = s1 / k, s2 / k
        var = mu2 - mu1 * mu1
        var = np.where(var > 0, var, F(0))
        V = np.where(spatial, var / n_out, own / n_out)
    assert V.dtype == np.float32 and k.dtype == np.float32
    return V, spatial, k


def denoise(C, m2, n, A, N, P, hit, hist, cam, cap=64.0, levels=5, sigma_l=4.0, sigma_z=0.1, motion=None, window=True):
    """One moments call: (result (H, W, 3), n_out (H, W), the history a commit leaves, dict(D, S, V, spatial, k)).  cam = (origin, inv_proj, inv_view)
    of this call; hist: what the last committing call of ANY kind left (a plain call's is not found); motion: None, or (tri, uv, cur) of a call that
    follows moved geometry (temporal_motion_truth.denoise's arguments)."""
    C = np.asarray(C, np.float32)
    h, w = C.shape[:2]
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    A, N, P = (np.ascontiguousarray(v, np.float32) for v in (A, N, P))
    hit = np.asarray(hit).astype(bool)
    hist = history_for(hist, True)
    D0, S0, ka = prepare(C, m2, n, A)
    through = None
    if motion is not None:
        tri, uv, cur = motion
        Pp, _, Np, valid = TM.previous_point(None if hist is None else hist.get("tris"), cur, tri, uv, N, P)
        through = (Np, Pp, valid)
    Dm, Sm, n_out = merge(D0, S0, n, N, P, A, hit, hist, cap, through)
    V, spatial, k = variance(Dm, Sm, n_out, N, P, A, hit, cam[0], window)
    Df, Vf = Dm, V
    for i in range(levels):
        Df, Vf = D.level(Df, Vf, N, P, hit, 1 << i, sigma_l, sigma_z)
    with np.errstate(all="ignore"):
        out = Df * ka
    assert out.dtype == np.float32
    new = TT.commit(Dm, Sm, n_out, N, P, A, hit, *cam)
    new["moments"] = True
    if motion is not None:
        new["tris"] = np.array(motion[2], np.float32).reshape(-1, TM.TRI_WORDS).copy()
    return out, n_out, new, dict(D=Dm, S=Sm, V=V, spatial=spatial, k=k)
