"""The truth the specular-guide tests use (not a test module): csrc/device/guide_chain.hpp restated in numpy float32 — the operations in the written
order, no fma — over what the CPU ORACLE gives: its primary frames of types 0 / 4 / 5 and O.trace for every bounce's closest hit.  A textured
surface's albedo is O.sample_texture at the shading's texture coordinates, whose fma is emulated in long double as tests/noise_truth.py does.
Also the class-aware a-trous level: tests/denoise_truth.py's level with `class == class` in place of `hit == hit`."""
import numpy as np

from oracle import oracle_py as O
from tests import denoise_truth as D

F = np.float32
FINITE_MAX = F(3.0e38)
MAX_BOUNCES = 8


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize(v):
    """(v / |v|, ok): (0, 0, 0) and False where |v|^2 is not in (0, 3e38]."""
    with np.errstate(all="ignore"):
        len2 = dot(v, v)
        ok = (len2 > 0) & (len2 <= FINITE_MAX)
        ln = np.sqrt(len2)
        out = np.where(ok[..., None], v / ln[..., None], F(0)).astype(np.float32)
    return out, ok


def direction_ok(d):
    with np.errstate(all="ignore"):
        len2 = dot(d, d)
        return (len2 > 0) & (len2 <= FINITE_MAX)


def reflect(d, n):
    k = F(2.0) * dot(d, n)
    return d - k[..., None] * n


def mirror(d, n):
    flip = dot(d, n) > 0
    return reflect(d, np.where(flip[..., None], -n, n))


def dielectric(d, n, ior):
    """(next direction, refracted?)"""
    with np.errstate(all="ignore"):
        cosi = dot(d, n)
        out = cosi > 0
        etai, etat = np.where(out, ior, F(1.0)).astype(np.float32), np.where(out, F(1.0), ior).astype(np.float32)
        n = np.where(out[..., None], n, -n)
        cosi = np.where(out, cosi, -cosi)
        eta = etai / etat
        cos2 = F(1.0) - (eta * eta) * (F(1.0) - cosi * cosi)
        refracted = cos2 > 0
        k = eta * cosi + np.sqrt(cos2)
        r, _ = normalize(d * eta[..., None] + n * k[..., None])
        nxt = np.where(refracted[..., None], r, reflect(d, n)).astype(np.float32)
    return nxt, refracted


def hit_point(tri, u, v):
    """tri: (n, 18) words 0..17 of the records; -> (P, N): p0 by u, p1 by v, p2 by w, the normal normalised (zero where it cannot be)."""
    u, v = u[:, None], v[:, None]
    w = (F(1.0) - u) - v
    p = (tri[:, 0:3] * u + tri[:, 3:6] * v) + tri[:, 6:9] * w
    m = (tri[:, 9:12] * u + tri[:, 12:15] * v) + tri[:, 15:18] * w
    return p.astype(np.float32), normalize(m.astype(np.float32))[0]


class NumpyOps:
    """guide_chain.hpp's chain_at_primary and chain_at_surface over arrays."""

    def at_surface(self, T, d, L, bad, illum, kd, ks, ior, n, K):
        """-> go, albedo of a chain that ends here, next direction, next throughput"""
        delta = ~bad & (illum >= 3) & (illum <= 7)
        is_mirror = (illum >= 3) & (illum <= 5)
        with np.errstate(all="ignore"):
            sm = np.where(is_mirror[:, None], ks, F(1.0)).astype(np.float32)
            albedo = np.where(delta[:, None], T * sm, T * kd).astype(np.float32)
            nxt = np.where(is_mirror[:, None], mirror(d, n), dielectric(d, n, ior)[0]).astype(np.float32)
        go = delta & (L < K) & direction_ok(nxt)
        return go, albedo, np.where(go[:, None], nxt, d).astype(np.float32), np.where(go[:, None], albedo, T).astype(np.float32)

    def at_primary(self, bad, illum, ks, ior, n, p, origin, K):
        """-> go, direction, throughput"""
        cnt = len(illum)
        d0, ok = normalize((p - np.asarray(origin, np.float32)[None, :]).astype(np.float32))
        delta = ~bad & (illum >= 3) & (illum <= 7)
        T = np.ones((cnt, 3), np.float32)
        go, _, d, T2 = self.at_surface(T, d0, np.zeros(cnt, np.int32), bad, illum, np.zeros((cnt, 3), np.float32), ks, ior, n, K)
        go = go & delta & ok
        return go, np.where(go[:, None], d, F(0)).astype(np.float32), np.where(go[:, None], T2, F(1.0)).astype(np.float32)


def materials_of(osc, tri):
    """bad, illum, kd (untextured), ks, ior, dtex of the triangles `tri`"""
    mats = osc.materials
    matid = osc.triangles["matid"][tri]
    bad = (matid < 0) | (matid >= len(mats))
    m = mats[np.where(bad, 0, matid)]
    z3 = np.zeros((len(tri), 3), np.float32)
    return (bad, np.where(bad, 0, m["illum"]).astype(np.int32), np.where(bad[:, None], z3, m["kd"]).astype(np.float32), np.where(bad[:, None], z3, m["ks"]).astype(np.float32),
            np.where(bad, F(1.0), m["ior"]).astype(np.float32), np.where(bad, -1, m["dtex"]).astype(np.int32))


def fma(a, b, c):
    return (a.astype(np.longdouble) * b.astype(np.longdouble) + c.astype(np.longdouble)).astype(np.float32)


def textured_kd(osc, tri, u, v, kd, dtex):
    """the shading's diffuse colour: the texture's where the material has one (shade.hpp fetch_info / textured_diffuse)"""
    kd = kd.copy()
    n_tex = len(osc.textures)
    use = (n_tex != 0) & (dtex != -1) & (dtex >= 0) & (dtex < n_tex)
    if not use.any():
        return kd
    tc = osc.triangles["tc"][tri]  # (n, 3, 2)
    w = (F(1.0) - u) - v
    s = fma(tc[:, 2, 0], w, fma(tc[:, 1, 0], v, tc[:, 0, 0] * u))
    t = fma(tc[:, 2, 1], w, fma(tc[:, 1, 1], v, tc[:, 0, 1] * u))
    for k in np.unique(dtex[use]):
        sel = use & (dtex == k)
        kd[sel] = O.sample_texture(osc.textures[int(k)], s[sel], t[sel])
    return kd


def tri_words(osc, tri):
    t = osc.triangles[tri]
    return np.concatenate([t["p"].reshape(-1, 9), t["n"].reshape(-1, 9)], axis=1).astype(np.float32)


def primary_guides(osc, P):
    frames = [O.primary_frame(osc, P, t) for t in (0, 4, 5)]
    h = frames[0][1]
    return dict(albedo=frames[0][0][..., :3].copy(), normal=frames[1][0][..., :3].copy(), position=frames[2][0][..., :3].copy(), tri=h["tri_id"].copy(), u=h["u"].copy(), v=h["v"].copy())


def chain_guides(osc, P, K, primary=None, ops=None):
    """-> dict(albedo, normal, position (H, W, 3) float32, chain (H, W) int8, hit (H, W) bool, rays, followed, escaped, truncated)."""
    assert 1 <= K <= MAX_BOUNCES
    ops = ops or NumpyOps()
    g = primary or primary_guides(osc, P)
    h, w = g["tri"].shape
    A, Nn, Pp = (g[k].reshape(-1, 3).copy() for k in ("albedo", "normal", "position"))
    tri0 = g["tri"].reshape(-1)
    cls = np.where(tri0 != -1, 1, 0).astype(np.int8)
    pix = np.flatnonzero(tri0 != -1)
    bad, illum, kd, ks, ior, dtex = materials_of(osc, tri0[pix])
    origin = np.array(list(P.origin), np.float32)
    go, d, T = ops.at_primary(bad, illum, ks, ior, Nn[pix], Pp[pix], origin, K)
    pix, d, T, p = pix[go], d[go], T[go], Pp[pix][go]
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
        pix, d, T, L, hits = pix[keep], d[keep], T[keep], L[keep] + 1, hits[keep]
        if len(pix) == 0:
            break
        tri = hits["tri_id"]
        p, n = getattr(ops, "hit_point", hit_point)(tri_words(osc, tri), hits["u"].copy(), hits["v"].copy())
        bad, illum, kd, ks, ior, dtex = materials_of(osc, tri)
        delta = ~bad & (illum >= 3) & (illum <= 7)
        kd = textured_kd(osc, tri, hits["u"], hits["v"], kd, np.where(delta, -1, dtex))
        go, albedo, d, T = ops.at_surface(T, d, L, bad, illum, kd, ks, ior, n, K)
        e = pix[~go]
        A[e], Nn[e], Pp[e], cls[e] = albedo[~go], n[~go], p[~go], 1 + L[~go]
        counts["truncated"] += int((~go & delta).sum())
        pix, d, T, L, p = pix[go], d[go], T[go], L[go], p[go]
    assert len(pix) == 0, "a chain outlived its bounces"
    out = dict(albedo=A.reshape(h, w, 3), normal=Nn.reshape(h, w, 3), position=Pp.reshape(h, w, 3), chain=cls.reshape(h, w), hit=(cls != 0).reshape(h, w))
    out.update(counts)
    return out


# ---- one kernel's part of the chain: what k_chain_start does per pixel and k_chain_step per ray, composed from the operations above ----
def start(osc, tri, normal, position, origin, K, ops=None, unfold=None):
    """The start of the chain at every pixel given: tri (n,) int32 the primary hit words (a word outside [0, triangles) is no known triangle), normal and
    position (n, 3) the captured guides.  -> dict(go (n,) bool: the pixel is followed; cls (n,) float32: the class of a pixel that is NOT followed (1 where
    the word is not -1, else 0); d, T (n, 3): the first ray's direction and the throughput of a followed pixel; length (n,): the unfolded length so far
    with `unfold` (virtual_truth.NumpyUnfold), 0 without)."""
    ops = ops or NumpyOps()
    tri = np.asarray(tri, np.int32)
    cnt = len(tri)
    normal, position = np.asarray(normal, np.float32).reshape(cnt, 3), np.asarray(position, np.float32).reshape(cnt, 3)
    go, d, T, length = np.zeros(cnt, bool), np.zeros((cnt, 3), np.float32), np.ones((cnt, 3), np.float32), np.zeros(cnt, np.float32)
    at = np.flatnonzero((tri >= 0) & (tri < len(osc.triangles)))
    if len(at):
        bad, illum, _, ks, ior, _ = materials_of(osc, tri[at])
        go[at], d[at], T[at] = ops.at_primary(bad, illum, ks, ior, normal[at], position[at], origin, K)
    if unfold is not None and go.any():
        length[go] = unfold.start_length(position[go], origin)
    return dict(go=go, cls=np.where(tri != -1, F(1), F(0)).astype(np.float32), d=d, T=T, length=length)


def step(osc, tri, u, v, T, d, L, K, ray_origin=None, length=None, ops=None, unfold=None):
    """One round of the chain for the rays given: tri (n,) int32 the closest-hit words the traversal answered, (u, v) of the hits, (T, d, L) the state
    the rays were traced with and, with `unfold`, ray_origin (n, 3) and length (n,) so far.  -> dict(go: the chain goes on; escaped, truncated (n,) bool;
    albedo, normal, position (n, 3) and cls (n,) int32: the guides of a chain that ended (where ~go); p: the hit point, d, T, L, length: the state and
    the next ray's origin where go)."""
    ops = ops or NumpyOps()
    tri, L = np.asarray(tri, np.int32), np.asarray(L, np.int32)
    cnt = len(tri)
    T, d = np.asarray(T, np.float32).reshape(cnt, 3), np.asarray(d, np.float32).reshape(cnt, 3)
    escaped = ~((tri >= 0) & (tri < len(osc.triangles)))
    out = dict(go=np.zeros(cnt, bool), escaped=escaped, truncated=np.zeros(cnt, bool), albedo=T.copy(), normal=d.copy(), position=np.zeros((cnt, 3), np.float32),
               cls=(-(L + 1)).astype(np.int32), p=np.zeros((cnt, 3), np.float32), d=d.copy(), T=T.copy(), L=L.copy(),
               length=np.zeros(cnt, np.float32) if length is None else np.asarray(length, np.float32).copy())
    at = np.flatnonzero(~escaped)
    if len(at) == 0:
        return out
    L1 = L[at] + 1
    p, n = getattr(ops, "hit_point", hit_point)(tri_words(osc, tri[at]), np.asarray(u, np.float32)[at].copy(), np.asarray(v, np.float32)[at].copy())
    if unfold is not None:
        out["length"][at] = unfold.unfold(out["length"][at], p, np.asarray(ray_origin, np.float32).reshape(cnt, 3)[at])
    bad, illum, kd, ks, ior, dtex = materials_of(osc, tri[at])
    delta = ~bad & (illum >= 3) & (illum <= 7)
    kd = textured_kd(osc, tri[at], np.asarray(u, np.float32)[at], np.asarray(v, np.float32)[at], kd, np.where(delta, -1, dtex))
    go, albedo, d2, T2 = ops.at_surface(T[at], d[at], L1, bad, illum, kd, ks, ior, n, K)
    out["go"][at], out["truncated"][at] = go, ~go & delta
    out["albedo"][at], out["normal"][at], out["position"][at], out["cls"][at] = albedo, n, p, 1 + L1
    out["p"][at], out["d"][at], out["T"][at], out["L"][at] = p, d2, T2, L1
    return out


def level(Dm, V, N, P, cls, step, sigma_l, sigma_z):
    """tests/denoise_truth.py level with a class per pixel: a tap counts where its class is the centre's; `hit` is class != 0."""
    sigma_l, sigma_z = F(sigma_l), F(sigma_z)
    h, w = V.shape
    cls = np.asarray(cls).astype(np.int32)
    hit = cls != 0
    H5, K3, lum, shifted = D.H5, D.K3, D.lum, D.shifted
    with np.errstate(all="ignore"):
        gs, gw = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                Vq, inside = shifted(V, dx, dy)
                cq, _ = shifted(cls, dx, dy)
                counts = inside & (cq == cls)
                k = K3[dx + 1] * K3[dy + 1]
                gs = np.where(counts, gs + k * Vq, gs)
                gw = np.where(counts, gw + k, gw)
        g = gs / gw
        sl = sigma_l * np.sqrt(g) + F(1e-4)
        Yp = lum(Dm)
        sw, sv, sd = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                Dq, inside = shifted(Dm, step * dx, step * dy)
                Vq, _ = shifted(V, step * dx, step * dy)
                cq, _ = shifted(cls, step * dx, step * dy)
                counts = inside & (cq == cls)
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
    assert D1.dtype == np.float32 and V1.dtype == np.float32
    return D1, V1


def denoise(C, m2, n, A, N, P, cls, levels=5, sigma_l=4.0, sigma_z=0.1):
    """tests/denoise_truth.py denoise with a class per pixel (classes {0, 1}: its bits)."""
    C = np.asarray(C, np.float32)
    h, w = C.shape[:2]
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    A, N, P = (np.ascontiguousarray(v, np.float32) for v in (A, N, P))
    Dm, V, ka = D.prepare(C, m2, n, A)
    for i in range(levels):
        Dm, V = level(Dm, V, N, P, cls, 1 << i, sigma_l, sigma_z)
    with np.errstate(all="ignore"):
        out = Dm * ka
    assert out.dtype == np.float32
    return out
