"""The truth the noise tests use (not a test module): exact per-frame samples from the CPU oracle, and the definition of
csrc/device/noise.hpp restated in numpy float32 / float64.

The oracle returns running means only, but called as frame 0 with the Sobol point of frame k (accum = 0: fmaf(0, 0, r) / 1 = r) it returns the exact clamped
sample of frame k — whenever frame k has sub-pixel index 0, i.e. subpixel == 1 or k < tmpLifetime (that call uses sub-pixel index 0 and re-traces the
primary ray)."""
import ctypes as C

import numpy as np

from oracle import oracle_py as O

F = np.float32
BLOCK = 32


def oracle_params(c, sun_visibility=False):
    ip, iv = O.camera(c.fov, c.yaw, c.pitch, c.width, c.height)
    return O.make_params(c.width, c.height, list(c.position), ip, iv, stack_size=c.stack_size, max_bounce=c.max_bounce, subpixel=c.subpixel,
                         tmp_life=c.tmp_lifetime, tmin=c.ray_tmin, clamp=c.clamp, sun=list(c.sun), sun_visibility=sun_visibility)


def frame_samples(osc, P, shift, sobol_matrices, n_frames):
    """(n_frames, H, W, 3) float32: the clamped sample of every frame.  Exact only under the condition above (asserted)."""
    assert P.subpixel == 1 or n_frames <= P.tmp_life, "no exact CPU samples beyond the first tmpLifetime group with sub-pixel jitter"
    shift = np.ascontiguousarray(shift, dtype=np.uint8)
    out = np.empty((n_frames, P.height, P.width, 3), dtype=np.float32)
    for k in range(n_frames):
        st = O.PathTracerState(P.width, P.height)
        pts = O.sobol(sobol_matrices, 2 * P.max_bounce, k, 1)
        O.lib().orc_pt_frames(C.byref(osc._c), C.byref(P), O._p(shift), O._p(pts), C.c_int(0), C.c_int(1), O._p(st.accum), O._p(st.cache_tri),
                              O._p(st.cache_uv), None, C.byref(O.Stats()), C.c_int(O.default_threads()))
        out[k] = st.accum[..., :3]
    return out


def running_mean(samples):
    """pathtracer.glsl:224-226 over the samples: fma(acc, k, r) / (k + 1), the fma emulated in long double (the product is exact, the sum rounds once at 64 bits
    before it rounds to 24: the check that uses this compares, it does not assume)."""
    acc = np.zeros(samples.shape[1:], dtype=np.float32)
    for k in range(samples.shape[0]):
        t = (acc.astype(np.longdouble) * np.longdouble(k) + samples[k].astype(np.longdouble)).astype(np.float32)
        acc = t / F(k + 1)
    return acc


def moments(samples, mean=None, m2=None, first=0):
    """noise.hpp noise_add_sample over frames first, first + 1, ...: (mean, m2), float32, in the written order, no fma."""
    mean = np.zeros(samples.shape[1:-1], dtype=np.float32) if mean is None else mean.copy()
    m2 = np.zeros(samples.shape[1:-1], dtype=np.float32) if m2 is None else m2.copy()
    for i in range(samples.shape[0]):
        r = samples[i]
        n = F(first + i + 1)
        y = (F(0.2126) * r[..., 0] + F(0.7152) * r[..., 1]) + F(0.0722) * r[..., 2]
        d = y - mean
        mean = mean + d / n
        m2 = m2 + d * (y - mean)
    assert mean.dtype == np.float32 and m2.dtype == np.float32
    return mean, m2


def noise_e(mean, m2, n_frames):
    """noise.hpp noise_of_pixel."""
    n = F(n_frames)
    e = np.sqrt(m2 / (n * (n - F(1.0)))) / (mean + F(0.01))
    assert e.dtype == np.float32
    return e


def blocks(e):
    """(index, sum float64, count) of every 32x32 block of the H x W image, ascending block index; the pixels inside the image only."""
    h, w = e.shape
    nbx, nby = (w + BLOCK - 1) // BLOCK, (h + BLOCK - 1) // BLOCK
    idx, s, cnt = [], [], []
    for by in range(nby):
        for bx in range(nbx):
            t = e[by * BLOCK:(by + 1) * BLOCK, bx * BLOCK:(bx + 1) * BLOCK].astype(np.float64)
            idx.append(by * nbx + bx); s.append(t.sum()); cnt.append(t.size)
    return np.array(idx, np.int32), np.array(s, np.float64), np.array(cnt, np.uint32)


def image_numbers(idx, s, cnt, pixels):
    """mean_noise, worst_block, worst_index (lowest index on a tie), and the gap between the two largest block means."""
    total = 0.0
    for v in s:  # ascending block index
        total += float(v)
    means = s / cnt
    worst = int(np.argmax(means))  # (the first of equal maxima)
    order = np.sort(means)
    gap = float(order[-1] - order[-2]) if len(order) > 1 else float("inf")
    return total / float(pixels), float(means[worst]), int(idx[worst]), gap


def truth(samples, n_frames):
    """Everything the library reports after n_frames frames."""
    mean, m2 = moments(samples[:n_frames])
    e = noise_e(mean, m2, n_frames)
    idx, s, cnt = blocks(e)
    mean_noise, worst_block, worst_index, gap = image_numbers(idx, s, cnt, e.size)
    return dict(mean=mean, m2=m2, e=e, idx=idx, sum=s, count=cnt, mean_noise=mean_noise, worst_block=worst_block, worst_index=worst_index, gap=gap)
