"""The pre-split of large triangles (adypt_amd/csrc/device/presplit.hpp) restated in numpy float32, a depth at a time over whole arrays: the same
thresholds, the same cut (the middle of the longest axis, the first axis wins ties), the same Sutherland-Hodgman clip (plane order, edge order, the
crossing point a + t * (b - a) with its coordinate on the plane set to the plane), the same pad and clamps, the same histogram and level.  Not a
translation of the header's walk: that one goes depth first with a stack per triangle, this one keeps every cell of a depth in arrays and orders the
leaves afterwards by their paths, low half first.  min / max are taken on the integer keys that order the binary32 values (tests/refit_truth.py)."""
import numpy as np

from oracle import oracle_py as O
from tests import refit_truth as T

LEVELS, MAX_DEPTH, POLYGON = 24, 6, 9
F = np.float32


def area(lo, hi):
    """cut_area: (ex * (ey + ez) + ey * ez) * 2 in binary32, the operations in that order"""
    with np.errstate(invalid="ignore", over="ignore"):
        e = (hi - lo).astype(F)
        return ((e[..., 0] * (e[..., 1] + e[..., 2]).astype(F)).astype(F) + (e[..., 1] * e[..., 2]).astype(F)).astype(F) * F(2.0)


def threshold(s, level):
    return F(s) * F(2.0 ** -level)


def positions(triangles):
    return np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1)["p"].astype(F)


def boxes(p):
    k = T.key(p)
    return T.unkey(k.min(axis=1)), T.unkey(k.max(axis=1))


def scene_area(p):
    k = T.key(p.reshape(-1, 3))
    return area(T.unkey(k.min(axis=0)), T.unkey(k.max(axis=0)))


def clip_plane(poly, cnt, k, plane, keep_above):
    """one plane over N polygons at once: poly [N, 9, 3], cnt [N], k [N] the axis, plane [N]; in the polygons' own number format"""
    F = poly.dtype.type
    n = len(poly)
    rows = np.arange(n)
    out, m = np.zeros_like(poly), np.zeros(n, np.int64)
    for i in range(POLYGON):
        active = i < cnt
        h = np.where(i == 0, cnt - 1, i - 1).clip(0, POLYGON - 1)
        a, b = poly[rows, h], poly[:, i]
        ak, bk = a[rows, k], b[rows, k]
        a_in = (ak >= plane) if keep_above else (ak <= plane)
        b_in = (bk >= plane) if keep_above else (bk <= plane)
        cross = active & (a_in != b_in)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            t = ((plane - ak).astype(F) / (bk - ak).astype(F)).astype(F)
            pt = (a + (t[:, None] * (b - a).astype(F)).astype(F)).astype(F)
        pt[rows, k] = plane
        w = np.nonzero(cross & (m < POLYGON))[0]  # (a vertex beyond the ninth is dropped: a convex polygon never has one)
        out[w, m[w]] = pt[w]
        m[w] += 1
        w = np.nonzero(active & b_in & (m < POLYGON))[0]
        out[w, m[w]] = b[w]
        m[w] += 1
    return out, m


def clip(p, half_lo, half_hi, whole_lo, whole_hi, pad):
    """presplit_clip over N triangles: (non-empty [N], lo [N, 3], hi [N, 3])"""
    n = len(p)
    poly, cnt = np.zeros((n, POLYGON, 3), F), np.full(n, 3, np.int64)
    poly[:, :3] = p
    for k in range(3):
        kk = np.full(n, k)
        poly, cnt = clip_plane(poly, cnt, kk, half_lo[:, k], True)
        poly, cnt = clip_plane(poly, cnt, kk, half_hi[:, k], False)
    valid = np.arange(POLYGON)[None, :, None] < cnt[:, None, None]
    key = T.key(poly)
    lo = T.unkey(np.where(valid, key, T.key(T.INF_LO)).min(axis=1))
    hi = T.unkey(np.where(valid, key, T.key(T.INF_HI)).max(axis=1))
    with np.errstate(invalid="ignore", over="ignore"):
        lo = T.unkey(np.maximum(np.maximum(T.key((lo - pad).astype(F)), T.key(half_lo)), T.key(whole_lo)))
        hi = T.unkey(np.minimum(np.minimum(T.key((hi + pad).astype(F)), T.key(half_hi)), T.key(whole_hi)))
    return cnt > 0, lo, hi


def walk(p, level_threshold, pad_scale=2.0 ** -20):
    """Every triangle's walk at one threshold.  Returns (the areas of the cells that split, leaves): leaves = (triangle, lo, hi, half_lo, half_hi) in
    reference order, half: the box the triangle was clipped against for this leaf (its own box for a triangle that is not split).  pad_scale: for
    measurements only — 0 shows what the unpadded binary32 clip gives."""
    whole_lo, whole_hi = boxes(p)
    pad = (np.abs(p).max(axis=1) * F(pad_scale)).astype(F)
    tri, lo, hi = np.arange(len(p)), whole_lo.copy(), whole_hi.copy()
    cell_lo, cell_hi = lo.copy(), hi.copy()
    path = np.zeros(len(p), np.int64)  # the halves taken so far, the first one highest: bit (MAX_DEPTH - depth) per step
    split_areas, leaves = [], []
    for depth in range(MAX_DEPTH + 1):
        a = area(lo, hi)
        with np.errstate(invalid="ignore"):
            cand = np.nonzero((a > level_threshold) & (depth < MAX_DEPTH))[0]
        splits = np.zeros(len(tri), bool)
        if len(cand):
            clo, chi, ct = lo[cand], hi[cand], tri[cand]
            e = (chi - clo).astype(F)
            k = np.where(e[:, 1] > e[:, 0], 1, 0)
            k = np.where(e[:, 2] > e[np.arange(len(cand)), k], 2, k)
            r = np.arange(len(cand))
            mid = ((clo[r, k] + chi[r, k]).astype(F) * F(0.5)).astype(F)
            low_hi, high_lo = chi.copy(), clo.copy()
            low_hi[r, k], high_lo[r, k] = mid, mid
            ok_l, l_lo, l_hi = clip(p[ct], clo, low_hi, whole_lo[ct], whole_hi[ct], pad[ct])
            ok_h, h_lo, h_hi = clip(p[ct], high_lo, chi, whole_lo[ct], whole_hi[ct], pad[ct])
            ok = ok_l & ok_h
            splits[cand[ok]] = True
            split_areas.append(a[cand[ok]])
        keep = ~splits
        leaves.append((tri[keep], path[keep], lo[keep], hi[keep], cell_lo[keep], cell_hi[keep]))
        if not splits.any():
            break
        w = cand[ok]
        bit = 1 << (MAX_DEPTH - 1 - depth)
        tri = np.concatenate([tri[w], tri[w]])
        path = np.concatenate([path[w], path[w] | bit])
        lo, hi = np.concatenate([l_lo[ok], h_lo[ok]]), np.concatenate([l_hi[ok], h_hi[ok]])
        cell_lo, cell_hi = np.concatenate([clo[ok], high_lo[ok]]), np.concatenate([low_hi[ok], chi[ok]])
    tri, path = np.concatenate([x[0] for x in leaves]), np.concatenate([x[1] for x in leaves])
    lo, hi = np.concatenate([x[2] for x in leaves]), np.concatenate([x[3] for x in leaves])
    cell_lo, cell_hi = np.concatenate([x[4] for x in leaves]), np.concatenate([x[5] for x in leaves])
    order = np.lexsort((path, tri))  # (leaves are no ancestors of each other: their paths, left-aligned, order them depth first, low half first)
    areas = np.concatenate(split_areas) if split_areas else np.zeros(0, F)
    return areas, (tri[order].astype(np.int32), lo[order], hi[order], cell_lo[order], cell_hi[order])


def allowed(budget, n):
    return int(np.floor(np.float64(budget) * np.float64(n)))


def histogram(p):
    s = scene_area(p)
    areas, _ = walk(p, threshold(s, LEVELS - 1))
    a_l = np.array([threshold(s, l) for l in range(LEVELS)], F)
    bins = (~(areas[:, None] > a_l[None, :])).sum(axis=1).clip(0, LEVELS - 1)  # the thresholds fall with l: the first l with area > A_l
    return np.bincount(bins, minlength=LEVELS).astype(np.int64), s


def refs(triangles, budget, hist=None):
    """(level, ref_tri int32 [r], ref_box float32 [r, 6]) of adypt_presplit_refs; hist: histogram(positions(triangles)), when the caller has it"""
    p = positions(triangles)
    n = len(p)
    whole_lo, whole_hi = boxes(p)
    level, extra = -1, 0
    if budget > 0:
        hist, s = hist if hist is not None else histogram(p)
        total = np.cumsum(hist)
        level = int((total <= allowed(budget, n)).sum()) - 1  # (the sums never fall: the levels inside the budget are the first ones)
        extra = int(total[level]) if level >= 0 else 0
    if extra == 0:
        return level, np.arange(n, dtype=np.int32), np.concatenate([whole_lo, whole_hi], axis=1)
    _, (tri, lo, hi, _, _) = walk(p, threshold(s, level))
    assert len(tri) == n + extra
    return level, tri, np.concatenate([lo, hi], axis=1)
