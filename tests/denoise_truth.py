"""The truth the denoiser tests use (not a test module): csrc/device/denoise.hpp restated in numpy float32 — the operations in the written order, no
fma, the selects as np.where(x > 0, x, 0), the taps that do not count skipped (an accumulator keeps its word, it is not given a zero to add)."""
import numpy as np

F = np.float32
BLOCK = 32
H5 = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]
K3 = [F(0.25), F(0.5), F(0.25)]


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def block_counts(h, w, per_block):
    """(H, W) float32 sample count of every pixel from the count of every 32x32 block (ascending block index), or from one number."""
    if np.ndim(per_block) == 0:
        return np.full((h, w), F(per_block), np.float32)
    nbx = (w + BLOCK - 1) // BLOCK
    yy, xx = np.mgrid[0:h, 0:w]
    return np.asarray(per_block)[(yy // BLOCK) * nbx + xx // BLOCK].astype(np.float32)


def shifted(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx], and which (y, x) have that tap inside the image."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((h, w), bool)
    ys, xs = slice(max(0, -dy), max(0, min(h, h - dy))), slice(max(0, -dx), max(0, min(w, w - dx)))
    yt, xt = slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)
    if ys.stop > ys.start and xs.stop > xs.start:
        b[ys, xs] = a[yt, xt]
        inside[ys, xs] = True
    return b, inside


def prepare(C, m2, n, A):
    C, m2, n, A = (np.asarray(v, np.float32) for v in (C, m2, n, A))
    with np.errstate(all="ignore"):
        V = m2 / (n * (n - F(1.0)))
        ka = A + F(0.01)
        D = C / ka
        la = lum(A) + F(0.01)
        V0 = V / (la * la)
    return D, V0, ka


def level(D, V, N, P, hit, step, sigma_l, sigma_z):
    sigma_l, sigma_z = F(sigma_l), F(sigma_z)
    h, w = V.shape
    hit = hit.astype(bool)
    with np.errstate(all="ignore"):
        gs, gw = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                Vq, inside = shifted(V, dx, dy)
                hq, _ = shifted(hit, dx, dy)
                counts = inside & (hq == hit)
                k = K3[dx + 1] * K3[dy + 1]
                gs = np.where(counts, gs + k * Vq, gs)
                gw = np.where(counts, gw + k, gw)
        g = gs / gw
        sl = sigma_l * np.sqrt(g) + F(1e-4)
        Yp = lum(D)
        sw, sv, sd = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                Dq, inside = shifted(D, step * dx, step * dy)
                Vq, _ = shifted(V, step * dx, step * dy)
                hq, _ = shifted(hit, step * dx, step * dy)
                counts = inside & (hq == hit)
                if dx == 0 and dy == 0:
                    wgt = np.full((h, w), H5[2] * H5[2], np.float32)
                else:
                    Nq, _ = shifted(N, step * dx, step * dy)
                    Pq, _ = shifted(P, step * dx, step * dy)
                    d = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                    t = np.where(d > 0, d, F(0))
                    for _ in range(5):
                        t = t * t
                    e = Pq - P
                    ln = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])
                    pd = np.abs((N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1]) + N[..., 2] * e[..., 2])
                    z = F(1.0) - pd / (sigma_z * ln + F(1e-6))
                    wz = np.where(z > 0, z, F(0))
                    t = np.where(hit, t, F(1.0)).astype(np.float32)
                    wz = np.where(hit, wz, F(1.0)).astype(np.float32)
                    xl = np.abs(lum(Dq) - Yp) / sl
                    wl = F(1.0) / (F(1.0) + xl * xl)
                    wgt = (((H5[dx + 2] * H5[dy + 2]) * t) * wz) * wl
                sw = np.where(counts, sw + wgt, sw)
                sd = np.where(counts[..., None], sd + wgt[..., None] * Dq, sd)
                sv = np.where(counts, sv + (wgt * wgt) * Vq, sv)
        D1 = sd / sw[..., None]
        V1 = sv / (sw * sw)
    assert D1.dtype == np.float32 and V1.dtype == np.float32 and sl.dtype == np.float32
    return D1, V1


def denoise(C, m2, n, A, N, P, hit, levels=5, sigma_l=4.0, sigma_z=0.1):
    """C (H, W, 3) radiance, m2 (H, W) luminance second moment, n the sample count (a number, or one per 32x32 block, or (H, W)), A / N / P (H, W, 3)
    the viewer colours of types 0 / 4 / 5, hit (H, W) bool  ->  (H, W, 3) float32."""
    C = np.asarray(C, np.float32)
    h, w = C.shape[:2]
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else block_counts(h, w, n)
    A, N, P = (np.ascontiguousarray(v, np.float32) for v in (A, N, P))
    hit = np.asarray(hit).astype(bool)
    D, V, ka = prepare(C, m2, n, A)
    for i in range(levels):
        D, V = level(D, V, N, P, hit, 1 << i, sigma_l, sigma_z)
    with np.errstate(all="ignore"):
        out = D * ka
    assert out.dtype == np.float32
    return out


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
