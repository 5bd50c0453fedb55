"""ctypes binding of adypt_amd/libadypt_probe.so (adypt_amd/csrc/probe/probe.h; not a test module): the device helpers of csrc/device one by one.
Test infrastructure like oracle/oracle_py.py — the product never loads that library.  Every function takes and returns numpy arrays, runs its
helper once per element on the GPU and raises on any HIP error."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

from oracle.oracle_py import MAT_DT

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(_ROOT, "adypt_amd", "csrc")
_LIB_PATH = os.path.join(_ROOT, "adypt_amd", "libadypt_probe.so")

F32, U32 = np.float32, np.uint32


def same(a, b):
    """Elementwise: equal bit patterns, or both NaN (sign and payload of a NaN differ legitimately between x86 and gfx950).  Signed zeros
    must match."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))


def _sources():
    return (glob.glob(os.path.join(_CSRC, "probe", "*")) + glob.glob(os.path.join(_CSRC, "device", "*.hpp")) +
            glob.glob(os.path.join(_CSRC, "device", "*.inc")) + glob.glob(os.path.join(_ROOT, "include", "adypt_h*.h")) + [os.path.join(_CSRC, "Makefile")])


def build(force=False):
    """(Re)build the library when it is missing or older than one of its sources; a failed build raises."""
    if force or not os.path.exists(_LIB_PATH) or os.path.getmtime(_LIB_PATH) < max(os.path.getmtime(s) for s in _sources()):
        subprocess.check_call(["make", "-C", _CSRC, "../libadypt_probe.so"], stdout=subprocess.DEVNULL)


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        from adypt_amd import _native  # noqa: F401  (settles which copy of the HIP runtime the process uses before this library binds to it)
        _lib = C.CDLL(_LIB_PATH)
    return _lib


def _call(name, *args):
    fn = getattr(lib(), "adypt_probe_" + name)
    fn.restype = C.c_int
    code = fn(*[a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in args])
    assert code == 0, "adypt_probe_%s: HIP error %d" % (name, -code)


def _f(a, cols=None):
    a = np.ascontiguousarray(a, dtype=F32)
    return a.reshape(-1) if cols is None else a.reshape(-1, cols)


def _u(a):
    return np.ascontiguousarray(a, dtype=U32).reshape(-1)


def _n(a):
    return C.c_int64(len(a))


def rcp(x):
    x = _f(x); out = np.empty_like(x)
    _call("rcp", x, out, _n(x))
    return out


def normalize(v):
    v = _f(v, 3); out = np.empty_like(v)
    _call("normalize", v, out, _n(v))
    return out


def sincos(x):
    x = _f(x); s = np.empty_like(x); c = np.empty_like(x)
    _call("sincos", x, s, c, _n(x))
    return s, c


def pow_(x, y):
    x, y = _f(x), _f(y); out = np.empty_like(x)
    assert len(x) == len(y)
    _call("pow", x, y, out, _n(x))
    return out


def unorm8(c):
    c = _u(c); out = np.empty(len(c), F32)
    _call("unorm8", c, out, _n(c))
    return out


def exp_byte(word):
    """(n, 3) uint32: the bits of exp_byte<0>, <1>, <2>."""
    word = _u(word); out = np.empty((len(word), 3), U32)
    _call("exp_byte", word, out, _n(word))
    return out


def shl_bytes(s, x):
    """(n, 4) uint32: shl_bytes<0..3>(s, x)."""
    s, x = _u(s), _u(x); out = np.empty((len(s), 4), U32)
    assert len(s) == len(x)
    _call("shl_bytes", s, x, out, _n(s))
    return out


def or_if_le(A, a, b, bits, B, lane_mask):
    A, a, b, bits, B = _u(A), _f(a), _f(b), _u(bits), _u(B)
    assert len(A) == len(a) == len(b) == len(bits) == len(B)
    out = np.empty(len(A), U32)
    _call("or_if_le", A, a, b, bits, B, C.c_uint64(lane_mask), out, _n(A))
    return out


def minmax(a, b):
    """(n, 4): max_num, min_num, gl_min, gl_max of (a, b)."""
    a, b = _f(a), _f(b); out = np.empty((len(a), 4), F32)
    assert len(a) == len(b)
    _call("minmax", a, b, out, _n(a))
    return out


def pk_fma_hi(a, b, c):
    """(pk_fma_hi(a, b, c), pk_fma(a, v2s(b.y), c)), each (n, 2)."""
    a, b, c = _f(a, 2), _f(b, 2), _f(c, 2)
    assert len(a) == len(b) == len(c)
    hi, plain = np.empty_like(a), np.empty_like(a)
    _call("pk_fma_hi", a, b, c, hi, plain, _n(a))
    return hi, plain


def sobol2(q, s):
    """Sobol point q + shift s, through both overloads (Rng reading the point from device memory, RngPoint): two (n, 2) arrays."""
    q, s = _f(q, 2), _f(s, 2)
    assert len(q) == len(s)
    o1, o2 = np.empty_like(q), np.empty_like(q)
    _call("sobol2", q, s, o1, o2, _n(q))
    return o1, o2


def sample_hemisphere(r, e):
    r = _f(r, 2); out = np.empty((len(r), 3), F32)
    _call("sample_hemisphere", r, C.c_float(e), out, _n(r))
    return out


def align_direction(direction, target):
    d, t = _f(direction, 3), _f(target, 3); out = np.empty_like(d)
    assert len(d) == len(t)
    _call("align_direction", d, t, out, _n(d))
    return out


def respond(materials, normal, dir_in, r, max_bounce=8):
    """respond<RngPoint> at bounce 0, colour 1 and radiance 0 going in: (direction (n, 3), throughput (n, 3), ret (n, 3), alive bool (n))."""
    m = np.ascontiguousarray(materials)
    assert m.dtype == MAT_DT
    nrm, d, rr = _f(normal, 3), _f(dir_in, 3), _f(r, 2)
    assert len(m) == len(nrm) == len(d) == len(rr)
    do, co, ro, al = np.empty_like(d), np.empty_like(d), np.empty_like(d), np.empty(len(m), np.int32)
    _call("respond", m, nrm, d, rr, C.c_int(max_bounce), do, co, ro, al, _n(m))
    assert np.isin(al, (0, 1)).all()
    return do, co, ro, al == 1


def sample_texture(rgb, s, t):
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    s, t = _f(s), _f(t); out = np.empty((len(s), 3), F32)
    assert len(s) == len(t)
    _call("sample_texture", rgb, C.c_int(rgb.shape[1]), C.c_int(rgb.shape[0]), s, t, out, _n(s))
    return out


def display(rgba, viewer_type):
    """k_display: (n, 4) float32 -> (n, 4) uint8 (R, G, B, A)."""
    rgba = _f(rgba, 4); out = np.empty(len(rgba), U32)
    _call("display", rgba, C.c_int(viewer_type), out, _n(rgba))
    return out.view(np.uint8).reshape(-1, 4)


# ---- the denoiser's kernels (csrc/device/denoise_kernels.hpp), each launched as denoise.hip launches it ----
UNWRITTEN = 0x7fc0dead  # the word every output holds before the launch


def unwritten(a):
    """Elementwise: the word is still the one the probe filled the output with — no thread wrote it."""
    return np.ascontiguousarray(a, dtype=F32).view(U32) == U32(UNWRITTEN)


def _img(a, h, w, c=4):
    a = np.ascontiguousarray(a, dtype=F32)
    assert a.shape == (h, w, c), (a.shape, (h, w, c))
    return a


def _local(a, n_blocks, c=4):
    a = np.ascontiguousarray(a, dtype=F32)
    assert a.shape == (n_blocks * 1024, c), (a.shape, n_blocks, c)
    return a


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def denoise_prepare(accum, moments, albedo, normal, position, hits, blocks, block_spp, w, h):
    """k_denoise_prepare over block-major arrays ((n_blocks * 1024, 4) float32; moments (., 2); hits with the triangle index as the bits of .x) of the
    block list given: X0, X1, X2, XA, each (h, w, 4)."""
    blocks, block_spp = _i32(blocks), _i32(block_spp)
    nb = len(blocks)
    assert len(block_spp) == nb
    out = [np.empty((h, w, 4), F32) for _ in range(4)]
    _call("denoise_prepare", _local(accum, nb), _local(moments, nb, 2), _local(albedo, nb), _local(normal, nb), _local(position, nb), _local(hits, nb), blocks, block_spp, C.c_int(nb),
          C.c_int(w), C.c_int(h), *out)
    return out


def atrous(x0, x1, x2, xa, step, sigma_l, sigma_z, last):
    """k_atrous<last>: the next X0 (h, w, 4), or the result (h, w, 3)."""
    h, w = np.shape(x0)[:2]
    out = np.empty((h, w, 3 if last else 4), F32)
    _call("atrous", _img(x0, h, w), _img(x1, h, w), _img(x2, h, w), _img(xa, h, w), C.c_int(w), C.c_int(h), C.c_int(step), C.c_float(sigma_l), C.c_float(sigma_z), C.c_int(1 if last else 0), out)
    return out


def rectify_window(radius, x0, x1, x2, xa, origin):
    """k_rectify_window<radius>: R0, R1 (h, w, 4)."""
    h, w = np.shape(x0)[:2]
    r0, r1 = np.empty((h, w, 4), F32), np.empty((h, w, 4), F32)
    _call("rectify_window", C.c_int(radius), _img(x0, h, w), _img(x1, h, w), _img(x2, h, w), _img(xa, h, w), C.c_int(w), C.c_int(h), _f(origin), r0, r1)
    return r0, r1


def temporal_merge(x, hist, have, cam, cap, motion=None, rectify=None):
    """k_temporal_merge<motion is not None, rectify is not None>.  x = (X0, X1, X2, XA), hist = (H0, H1, H2, HA), cam = (origin, inv_proj, inv_view) of
    the history, motion = (XP, XN), rectify = (R0, R1, gamma): (merged (h, w, 4), X2 as the kernel leaves it, length (h, w), kept (h, w) or None)."""
    h, w = np.shape(x[0])[:2]
    x, hist = [_img(a, h, w) for a in x], [_img(a, h, w) for a in hist]
    o, ip, iv = (_f(v) for v in cam)
    assert len(o) == 3 and len(ip) == 16 and len(iv) == 16
    xp, xn = (_img(a, h, w) for a in motion) if motion is not None else (None, None)
    r0, r1 = (_img(a, h, w) for a in rectify[:2]) if rectify is not None else (None, None)
    merged, x2, length = np.empty((h, w, 4), F32), np.empty((h, w, 4), F32), np.empty((h, w), F32)
    kept = np.empty((h, w), F32) if rectify is not None else None
    _call("temporal_merge", C.c_int(motion is not None), C.c_int(rectify is not None), *x, *hist, C.c_int(1 if have else 0), o, ip, iv, C.c_float(cap), xp, xn, r0, r1,
          C.c_float(rectify[2] if rectify is not None else 0.0), C.c_int(w), C.c_int(h), merged, x2, length, kept)
    return merged, x2, length, kept


PREPARE_INSTANCES = {"class": 0, "moments": 1, "virtual": 2}  # probe.h ADYPT_PROBE_PREPARE_*


def denoise_prepare_instance(instance, accum, moments, albedo, normal, position, hits, blocks, block_spp, w, h, virtual=None):
    """k_denoise_prepare_class / _moments / _virtual over denoise_prepare's arrays (hits.w: the class word) and, for "virtual", the block-major image of
    the virtual points: X0, X1, X2, XA and, for "virtual", XV, each (h, w, 4)."""
    blocks, block_spp = _i32(blocks), _i32(block_spp)
    nb = len(blocks)
    assert len(block_spp) == nb and (virtual is not None) == (instance == "virtual")
    out = [np.empty((h, w, 4), F32) for _ in range(5 if instance == "virtual" else 4)]
    _call("denoise_prepare_instance", C.c_int(PREPARE_INSTANCES[instance]), _local(accum, nb), _local(moments, nb, 2), _local(albedo, nb), _local(normal, nb), _local(position, nb),
          _local(hits, nb), blocks, block_spp, C.c_int(nb), C.c_int(w), C.c_int(h), *out[:4], _local(virtual, nb) if virtual is not None else None, out[4] if virtual is not None else None)
    return out


def temporal_merge_moments(x, hist, have, cam, cap, motion=None):
    """k_temporal_merge_moments<motion is not None>: temporal_merge's arguments, the fourth channel of X0 and H0 holding S: (merged (h, w, 4), X2 as the
    kernel leaves it, length (h, w))."""
    h, w = np.shape(x[0])[:2]
    x, hist = [_img(a, h, w) for a in x], [_img(a, h, w) for a in hist]
    o, ip, iv = (_f(v) for v in cam)
    assert len(o) == 3 and len(ip) == 16 and len(iv) == 16
    xp, xn = (_img(a, h, w) for a in motion) if motion is not None else (None, None)
    merged, x2, length = np.empty((h, w, 4), F32), np.empty((h, w, 4), F32), np.empty((h, w), F32)
    _call("temporal_merge_moments", C.c_int(motion is not None), *x, *hist, C.c_int(1 if have else 0), o, ip, iv, C.c_float(cap), xp, xn, C.c_int(w), C.c_int(h), merged, x2, length)
    return merged, x2, length


def moments_variance(merged, x1, x2, xa, origin):
    """k_moments_variance: (out (h, w, 4) = (D, V), the variance read-out (h, w), the sum of the kernel's count slots)."""
    h, w = np.shape(merged)[:2]
    out, variance, count = np.empty((h, w, 4), F32), np.empty((h, w), F32), np.zeros(1, np.uint64)
    o = _f(origin)
    assert len(o) == 3
    _call("moments_variance", _img(merged, h, w), _img(x1, h, w), _img(x2, h, w), _img(xa, h, w), C.c_int(w), C.c_int(h), o, out, variance, count)
    return out, variance, int(count[0])


# ---- the chain through mirrors and glass: k_chain_start, k_chain_step ----
SEG_STRIDE = 16  # words between the counters of two segments of a queue


def device_materials(materials, texture=None):
    """(n, 20) float32: MAT_DT materials in the device's layout — the 64 bytes, then (texel offset, w, h, 0) of the diffuse texture where the material names
    the one texture there is (as upload_textures_and_materials leaves it)."""
    m = np.ascontiguousarray(materials).view(MAT_DT).reshape(-1)
    out = np.zeros((len(m), 20), U32)
    out[:, :16] = m.view(U32).reshape(len(m), 16)
    if texture is not None:
        out[m["dtex"] == 0, 16:19] = np.array([0, texture.shape[1], texture.shape[0]], U32)
    return out.view(F32)


def _scene_args(scene):
    """scene = (records (n_tris, 32), materials (n_mats, 20), texture (h, w, 3) uint8 or None)"""
    records, materials, texture = scene
    records, materials = np.ascontiguousarray(records).view(F32).reshape(-1, 32), np.ascontiguousarray(materials).view(F32).reshape(-1, 20)
    tex = None if texture is None else np.ascontiguousarray(texture, dtype=np.uint8)
    assert tex is None or (tex.ndim == 3 and tex.shape[2] == 3)
    return [records, C.c_int64(len(records)), materials, C.c_int(len(materials)), tex, C.c_int(0 if tex is None else tex.shape[1]), C.c_int(0 if tex is None else tex.shape[0])]


def chain_start(unfold, scene, albedo, normal, position, hits, blocks, w, h, origin, tmin, bounces, segments, seg_cap):
    """k_chain_start<unfold>: dict(albedo, normal, position, hits: the block-major guides as the kernel leaves them; state (n_px, 2, 4); o, d (segments,
    seg_cap, 4): the queue; count (segments,) and count_words (segments, 16): its counters; counts = dict(rays, followed, escaped, truncated))."""
    blocks = _i32(blocks)
    nb = len(blocks)
    g = [_local(a, nb).copy() for a in (albedo, normal, position, hits)]
    state, qo, qd = np.empty((nb * 1024, 2, 4), F32), np.empty((segments, seg_cap, 4), F32), np.empty((segments, seg_cap, 4), F32)
    qc, counts = np.empty((segments, SEG_STRIDE), U32), np.zeros(4, np.uint64)
    o = _f(origin)
    assert len(o) == 3
    _call("chain_start", C.c_int(1 if unfold else 0), *_scene_args(scene), *g, blocks, C.c_int(nb), C.c_int(w), C.c_int(h), o, C.c_float(tmin), C.c_int(bounces), C.c_int(segments),
          C.c_uint32(seg_cap), state, qo, qd, qc, counts)
    return dict(albedo=g[0], normal=g[1], position=g[2], hits=g[3], state=state, o=qo, d=qd, count=qc[:, 0].copy(), count_words=qc,
                counts=dict(zip(("rays", "followed", "escaped", "truncated"), (int(v) for v in counts))))


def chain_step(unfold, scene, albedo, normal, position, hits, state, queue, bounces, tmin, virt=None, origin=None):
    """k_chain_step<unfold>.  The guides (n_px, 4), state (n_px, 2, 4) and with unfold virt (n_px, 4); queue = dict(o, d, hit (segments, seg_cap, 4), count
    (segments,)).  -> dict(albedo, normal, position, hits, state, virt as the kernel leaves them; o, d, count, count_words: the queue it wrote; counts)."""
    n_px = len(hits)
    g = [np.ascontiguousarray(a, dtype=F32).reshape(n_px, 4).copy() for a in (albedo, normal, position, hits)]
    state = np.ascontiguousarray(state, dtype=F32).reshape(n_px, 2, 4).copy()
    qi = [np.ascontiguousarray(queue[k], dtype=F32) for k in ("o", "d", "hit")]
    segments, seg_cap = qi[0].shape[:2]
    assert all(a.shape == (segments, seg_cap, 4) for a in qi)
    ic = np.zeros((segments, SEG_STRIDE), U32)
    ic[:, 0] = queue["count"]
    qo, qd = np.empty((segments, seg_cap, 4), F32), np.empty((segments, seg_cap, 4), F32)
    qc, counts = np.empty((segments, SEG_STRIDE), U32), np.zeros(4, np.uint64)
    assert (virt is not None and origin is not None) or not unfold
    virt = np.ascontiguousarray(virt, dtype=F32).reshape(n_px, 4).copy() if unfold else None
    _call("chain_step", C.c_int(1 if unfold else 0), *_scene_args(scene), *g, C.c_int(n_px), C.c_int(segments), C.c_uint32(seg_cap), *qi, ic, C.c_int(bounces), C.c_float(tmin), state, qo,
          qd, qc, counts, virt, _f(origin) if unfold else None)
    return dict(albedo=g[0], normal=g[1], position=g[2], hits=g[3], state=state, virt=virt, o=qo, d=qd, count=qc[:, 0].copy(), count_words=qc,
                counts=dict(zip(("rays", "followed", "escaped", "truncated"), (int(v) for v in counts))))


def motion_gather(hits, normal, position, blocks, w, h, snapshot, records):
    """k_motion_gather: snapshot (n_known, 20) float32, records (n_records >= n_known, 4 * tri_float4): XP, XN (h, w, 4)."""
    blocks = _i32(blocks)
    nb = len(blocks)
    snapshot, records = np.ascontiguousarray(snapshot, dtype=F32), np.ascontiguousarray(records, dtype=F32)
    assert snapshot.ndim == 2 and snapshot.shape[1] == 20 and records.ndim == 2 and records.shape[1] % 4 == 0
    xp, xn = np.empty((h, w, 4), F32), np.empty((h, w, 4), F32)
    _call("motion_gather", _local(hits, nb), _local(normal, nb), _local(position, nb), blocks, C.c_int(nb), C.c_int(w), C.c_int(h), snapshot, C.c_int64(len(snapshot)), records,
          C.c_int64(len(records)), C.c_int(records.shape[1] // 4), xp, xn)
    return xp, xn


def motion_snapshot(records):
    """k_motion_snapshot: records (n, 4 * tri_float4) float32 -> (n, 20)."""
    records = np.ascontiguousarray(records, dtype=F32)
    assert records.ndim == 2 and records.shape[1] % 4 == 0
    out = np.empty((len(records), 20), F32)
    _call("motion_snapshot", records, C.c_int(records.shape[1] // 4), C.c_int64(len(records)), out)
    return out


def noise(samples, first, n_frames):
    """samples (n, k, 3): noise_add_sample folded over the k samples of every element as frames first, first + 1, ..., then
    noise_of_pixel(., n_frames): (mean, m2, e)."""
    s = np.ascontiguousarray(samples, dtype=F32)
    assert s.ndim == 3 and s.shape[2] == 3
    n, k = s.shape[0], s.shape[1]
    mean, m2, e = np.empty(n, F32), np.empty(n, F32), np.empty(n, F32)
    _call("noise", s, C.c_int(k), C.c_int(first), C.c_int(n_frames), mean, m2, e, C.c_int64(n))
    return mean, m2, e
