"""The truth the temporal-merge tests use (not a test module): csrc/device/temporal.hpp restated in numpy float32 — the operations in the written order,
no fma, a tap that does not count skipped (an accumulator keeps its word), every refusal written as `not (comparison)` so that a NaN refuses."""
import numpy as np

from tests import denoise_truth as D

F = np.float32
NORMAL_MIN, PLANE_TOL, ALBEDO_TOL, MIN_WEIGHT, FINITE_MAX = F(0.9), F(0.02), F(0.1), F(0.01), F(3.0e38)


def camera(origin, inv_proj, inv_view):
    """temporal_camera: o, a, b, c (3,) and the columns of R as rows of r (3, 3), all float32."""
    m, v = np.asarray(inv_proj, np.float32).reshape(16), np.asarray(inv_view, np.float32).reshape(16)
    return dict(o=np.asarray(origin, np.float32).reshape(3).copy(), a=m[0:3].copy(), b=m[4:7].copy(), c=(m[8:11] + m[12:15]).astype(np.float32),
                r=np.stack([v[0:3], v[4:7], v[8:11]]).astype(np.float32))


def reproject(cam, w, h, P):
    """(ok, fx, fy, dist) of every pixel's position under the history's camera."""
    o, a, b, c, r = cam["o"], cam["a"], cam["b"], cam["c"], cam["r"]
    with np.errstate(all="ignore"):
        e = [P[..., i] - o[i] for i in range(3)]
        dist = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        vx, vy, vz = [(r[k][0] * e[0] + r[k][1] * e[1]) + r[k][2] * e[2] for k in range(3)]
        m00, m01, r0 = a[0] * vz - a[2] * vx, b[0] * vz - b[2] * vx, c[2] * vx - c[0] * vz
        m10, m11, r1 = a[1] * vz - a[2] * vy, b[1] * vz - b[2] * vy, c[2] * vy - c[1] * vz
        det = m00 * m11 - m01 * m10
        ok = np.abs(det) > 0
        sx, sy = (r0 * m11 - m01 * r1) / det, (m00 * r1 - r0 * m10) / det
        tx, ty, tz = [(a[i] * sx + b[i] * sy) + c[i] for i in range(3)]
        ok &= ((tx * vx + ty * vy) + tz * vz) > 0
        fx = ((sx + F(1.0)) * F(w)) * F(0.5) - F(0.5)
        fy = ((F(1.0) - sy) * F(h)) * F(0.5) - F(0.5)
    assert fx.dtype == np.float32 and fy.dtype == np.float32 and dist.dtype == np.float32
    return ok, fx, fy, dist


def merge(D0, V0, n, N, P, A, hit, hist, cap=64.0):
    """The merged (D, V, n_out) of a call with the images given ((H, W, 3) / (H, W), n (H, W) float32); hist None, or what commit() made."""
    h, w = V0.shape
    D0, V0, n = np.asarray(D0, np.float32), np.asarray(V0, np.float32), np.asarray(n, np.float32)
    if hist is None:
        return D0.copy(), V0.copy(), n.copy()
    cap = F(cap)
    hit = np.asarray(hit).astype(bool)
    ok, fx, fy, dist = reproject(hist["cam"], w, h, P)
    with np.errstate(all="ignore"):
        ok = ok & hit & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
        fxs, fys = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        bx, by = np.floor(fxs), np.floor(fys)
        ix, iy = bx.astype(np.int64), by.astype(np.int64)
        ux, uy = fxs - bx, fys - by
        tol = PLANE_TOL * dist
        sw, sv, sn = (np.zeros((h, w), np.float32) for _ in range(3))
        sd = np.zeros((h, w, 3), np.float32)
        for ty in (0, 1):
            for tx in (0, 1):
                qx, qy = ix + tx, iy + ty
                counts = ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                Nq, Pq, Aq, Dq, Vq, nq = (hist[k][cy, cx] for k in ("N", "P", "A", "D", "V", "n"))
                counts &= hist["hit"][cy, cx].astype(bool)
                counts &= ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]) >= NORMAL_MIN
                d = Pq - P
                counts &= np.abs((N[..., 0] * d[..., 0] + N[..., 1] * d[..., 1]) + N[..., 2] * d[..., 2]) <= tol
                counts &= (np.abs(Aq - A) <= ALBEDO_TOL).all(-1)
                counts &= (np.abs(Dq) <= FINITE_MAX).all(-1) & (np.abs(Vq) <= FINITE_MAX) & (nq > 0) & (nq <= FINITE_MAX)
                wgt = ((F(1.0) - ux) if tx == 0 else ux) * ((F(1.0) - uy) if ty == 0 else uy)
                sw = np.where(counts, sw + wgt, sw)
                sd = np.where(counts[..., None], sd + wgt[..., None] * Dq, sd)
                sv = np.where(counts, sv + (wgt * wgt) * Vq, sv)
                sn = np.where(counts, sn + wgt * nq, sn)
        take = ok & (sw > MIN_WEIGHT)
        Dh, Vh, hq = sd / sw[..., None], sv / (sw * sw), sn / sw
        nh = np.where(hq < cap, hq, cap).astype(np.float32)
        den = n + nh
        Dm = (n[..., None] * D0 + nh[..., None] * Dh) / den[..., None]
        Vm = ((n * n) * V0 + (nh * nh) * Vh) / (den * den)
        Dm, Vm, no = np.where(take[..., None], Dm, D0), np.where(take, Vm, V0), np.where(take, den, n)
    assert Dm.dtype == np.float32 and Vm.dtype == np.float32 and no.dtype == np.float32
    return Dm, Vm, no


def commit(Dm, Vm, n_out, N, P, A, hit, origin, inv_proj, inv_view):
    return dict(D=Dm.copy(), V=Vm.copy(), n=n_out.copy(), N=np.array(N, np.float32), P=np.array(P, np.float32), A=np.array(A, np.float32),
                hit=np.asarray(hit).astype(bool).copy(), cam=camera(origin, inv_proj, inv_view))


def denoise(C, m2, n, A, N, P, hit, hist, cam, cap=64.0, levels=5, sigma_l=4.0, sigma_z=0.1):
    """One temporal call: (result (H, W, 3), n_out (H, W), the history a commit leaves).  cam = (origin, inv_proj, inv_view) of this call."""
    C = np.asarray(C, np.float32)
    h, w = C.shape[:2]
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    A, N, P = (np.ascontiguousarray(v, np.float32) for v in (A, N, P))
    hit = np.asarray(hit).astype(bool)
    D0, V0, ka = D.prepare(C, m2, n, A)
    Dm, Vm, n_out = merge(D0, V0, n, N, P, A, hit, hist, cap)
    Df, Vf = Dm, Vm
    for i in range(levels):
        Df, Vf = D.level(Df, Vf, N, P, hit, 1 << i, sigma_l, sigma_z)
    with np.errstate(all="ignore"):
        out = Df * ka
    assert out.dtype == np.float32
    return out, n_out, commit(Dm, Vm, n_out, N, P, A, hit, *cam)
