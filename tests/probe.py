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


def noise(samples, first, n_frames):
    """samples (n, k, 3): noise_add_sample folded over the k samples of every element as frames first, first + 1, ..., then
    noise_of_pixel(., n_frames): (mean, m2, e)."""
    s = np.ascontiguousarray(samples, dtype=F32)
    assert s.ndim == 3 and s.shape[2] == 3
    n, k = s.shape[0], s.shape[1]
    mean, m2, e = np.empty(n, F32), np.empty(n, F32), np.empty(n, F32)
    _call("noise", s, C.c_int(k), C.c_int(first), C.c_int(n_frames), mean, m2, e, C.c_int64(n))
    return mean, m2, e
