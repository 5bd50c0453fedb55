"""The truth the history-plan tests use (not a test module): csrc/device/history_reach.hpp restated — the reach in numpy float32 on top of
tests/temporal_truth.py (the operations in the written order, no fma, a tap that does not count skipped, every refusal written as `not (comparison)`
so that a NaN refuses), the bins, the plan of a block and the order of work in plain integers.  A history is what temporal_truth.commit makes."""
import numpy as np

from tests import temporal_motion_truth as TM
from tests import temporal_truth as TT

F = np.float32
BINS = 65


def reach(N, P, A, hit, hist, cap=64.0):
    """(H, W) float32: the length temporal_truth.merge adds to n at every pixel, 0 where it takes no history.  (N, P): what is reprojected and what
    the taps are held against."""
    hit = np.asarray(hit).astype(bool)
    h, w = hit.shape
    if hist is None:
        return np.zeros((h, w), np.float32)
    N, P, A = (np.asarray(v, np.float32) for v in (N, P, A))
    cap = F(cap)
    ok, fx, fy, dist = TT.reproject(hist["cam"], w, h, P)
    with np.errstate(all="ignore"):
        ok = ok & hit & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
        fxs, fys = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))
        bx, by = np.floor(fxs), np.floor(fys)
        ix, iy = bx.astype(np.int64), by.astype(np.int64)
        ux, uy = fxs - bx, fys - by
        tol = TT.PLANE_TOL * dist
        sw, sn = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
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
                sn = np.where(counts, sn + wgt * nq, sn)
        take = ok & (sw > TT.MIN_WEIGHT)
        hq = sn / sw
        nh = np.where(hq < cap, hq, cap).astype(np.float32)
        out = np.where(take, nh, F(0)).astype(np.float32)
    assert out.dtype == np.float32
    return out


def reach_motion(N, P, A, hit, hist, tri, uv, cur, cap=64.0):
    """The motion form: through temporal_previous_point of the hit triangle against the history's snapshot (hist["tris"], or none)."""
    prev = None if hist is None else hist.get("tris")
    Pp, _, Np, valid = TM.previous_point(prev, cur, tri, uv, N, P)
    return reach(Np, Pp, A, np.asarray(hit).astype(bool) & valid, hist, cap)


def blocks_of(w, h):
    """[(block index, y slice, x slice)] of the 32 x 32 blocks of the image, ascending block index."""
    nbx, nby = (w + 31) // 32, (h + 31) // 32
    return [(by * nbx + bx, slice(by * 32, min(h, by * 32 + 32)), slice(bx * 32, min(w, bx * 32 + 32))) for by in range(nby) for bx in range(nbx)]


def reach_bin(L):
    L = np.asarray(L, np.float32)
    return np.where(L >= F(64.0), 64, np.floor(np.minimum(L, F(64.0))).astype(np.int64)).astype(np.int64)


def bins(L, hit):
    """(blocks, 65) uint32: every block's hit pixels inside the image by the floor of their reach; bin 64: a reach of 64 or more."""
    L, hit = np.asarray(L, np.float32), np.asarray(hit).astype(bool)
    h, w = hit.shape
    out = np.zeros((len(blocks_of(w, h)), BINS), np.uint32)
    for b, ys, xs in blocks_of(w, h):
        out[b] = np.bincount(reach_bin(L[ys, xs][hit[ys, xs]]), minlength=BINS).astype(np.uint32)
    return out


def candidates(min_spp, max_spp, step):
    c = list(range(min_spp, max_spp, step))
    return c + [max_spp]


def plan_block(b, target, min_spp=2, max_spp=64, step=4, tolerance_permille=31):
    """The sample count of a block with the bins b: the smallest candidate that leaves at most hits * tolerance_permille // 1000 hit pixels with
    bin + n < target; max_spp if none does; min_spp for a block without a hit pixel."""
    b = [int(v) for v in b]
    hits = sum(b)
    if hits == 0:
        return min_spp
    allowed = hits * tolerance_permille // 1000
    for n in candidates(min_spp, max_spp, step):
        if sum(v for k, v in enumerate(b) if k + n < target) <= allowed:
            return n
    return max_spp


def plan(all_bins, target, min_spp=2, max_spp=64, step=4, tolerance_permille=31):
    return np.array([plan_block(b, target, min_spp, max_spp, step, tolerance_permille) for b in all_bins], np.int32)


def args_valid(target, min_spp, max_spp, step, tolerance_permille, history_cap):
    cap = np.float32(history_cap)
    return bool(1 <= target <= 1 << 20 and 2 <= min_spp <= max_spp and step >= 1 and 0 <= tolerance_permille <= 999 and cap > 0 and cap <= TT.FINITE_MAX)


def block_pixels(w, h):
    return np.array([(ys.stop - ys.start) * (xs.stop - xs.start) for _, ys, xs in blocks_of(w, h)], np.int64)


def pixel_samples(want, w, h):
    return int((block_pixels(w, h) * np.asarray(want, np.int64)).sum())


def per_pixel(want, w, h):
    """(H, W) int32: every pixel's block's count."""
    out = np.zeros((h, w), np.int32)
    for b, ys, xs in blocks_of(w, h):
        out[ys, xs] = want[b]
    return out


def order_of_work(want, start=0):
    """[("T", frames) | ("F", spp, [blocks])]: the distinct wants ascending, `want - counter` frames each, then the blocks of that want frozen at it —
    except the blocks of the largest, which stay active."""
    calls, counter = [], start
    distinct = sorted(set(int(v) for v in want))
    for k, n in enumerate(distinct):
        if n > counter:
            calls.append(("T", n - counter))
            counter = n
        if k + 1 < len(distinct):
            calls.append(("F", n, [b for b, v in enumerate(want) if int(v) == n]))
    return calls
