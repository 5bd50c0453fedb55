"""CPU test of libadypt_probe.so's entry checks (adypt_amd/csrc/probe/probe.h): a bad element count, size or null pointer is refused before
anything is allocated or launched, so these calls need no GPU.  What the probes compute is tests/test_gpu_device_probes.py's subject."""
import ctypes as C

import numpy as np

from tests import probe as P

INVALID = -1  # -hipErrorInvalidValue
ENTRIES = ("rcp", "normalize", "sincos", "pow", "unorm8", "exp_byte", "shl_bytes", "or_if_le", "minmax", "pk_fma_hi", "sobol2", "sample_hemisphere",
           "align_direction", "respond", "sample_texture", "display", "noise")


def test_every_entry_is_exported():
    for name in ENTRIES:
        assert hasattr(P.lib(), "adypt_probe_" + name), name


def test_bad_counts_sizes_and_null_pointers_are_refused():
    lib = P.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    for n, want in ((-1, INVALID), ((1 << 24) + 1, INVALID), (0, 0)):
        assert lib.adypt_probe_rcp(p, p, C.c_int64(n)) == want
        assert lib.adypt_probe_pow(p, p, p, C.c_int64(n)) == want
        assert lib.adypt_probe_or_if_le(p, p, p, p, p, C.c_uint64(1), p, C.c_int64(n)) == want
        assert lib.adypt_probe_respond(p, p, p, p, C.c_int(8), p, p, p, p, C.c_int64(n)) == want
        assert lib.adypt_probe_display(p, C.c_int(0), p, C.c_int64(n)) == want
    assert lib.adypt_probe_rcp(None, p, C.c_int64(4)) == INVALID and lib.adypt_probe_sincos(p, p, None, C.c_int64(4)) == INVALID
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 24, 2)):
        assert lib.adypt_probe_sample_texture(p, C.c_int(w), C.c_int(h), p, p, p, C.c_int64(4)) == INVALID
    for k, first in ((-1, 0), (4097, 0), (4, -1), (4, 2 ** 31 - 2)):
        assert lib.adypt_probe_noise(p, C.c_int(k), C.c_int(first), C.c_int(2), p, p, p, C.c_int64(4)) == INVALID
    assert lib.adypt_probe_noise(p, C.c_int(4096), C.c_int(0), C.c_int(2), p, p, p, C.c_int64(1 << 13)) == INVALID  # n * k beyond 2^24 samples


KERNEL_ENTRIES = ("denoise_prepare", "atrous", "rectify_window", "temporal_merge", "motion_gather", "motion_snapshot")


def test_the_denoiser_kernel_entries_refuse_what_a_kernel_must_not_be_given():
    """A block outside the picture's grid, a hit word farther than 32 from the snapshot, a radius, a step or a picture size out of range: refused before
    anything is allocated or launched — a kernel writes where the block list says and the gather reads where a hit word says."""
    lib = P.lib()
    for name in KERNEL_ENTRIES:
        assert hasattr(lib, "adypt_probe_" + name), name
    buf = np.zeros(4 * 1024, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    i = C.c_int
    spp = np.array([8], np.int32).ctypes.data_as(C.c_void_p)
    for block, w, h in ((-1, 8, 8), (1, 8, 8), (2, 33, 9), (0, 0, 8), (0, 8, 4097)):
        blocks = np.array([block], np.int32)
        b = blocks.ctypes.data_as(C.c_void_p)
        assert lib.adypt_probe_denoise_prepare(p, p, p, p, p, p, b, spp, i(1), i(w), i(h), p, p, p, p) == INVALID, (block, w, h)
        assert lib.adypt_probe_motion_gather(p, p, p, b, i(1), i(w), i(h), p, C.c_int64(0), p, C.c_int64(4), i(5), p, p) == INVALID, (block, w, h)
    zero = np.array([0], np.int32).ctypes.data_as(C.c_void_p)
    assert lib.adypt_probe_denoise_prepare(p, p, p, p, p, p, zero, spp, i(0), i(8), i(8), p, p, p, p) == INVALID and lib.adypt_probe_denoise_prepare(p, p, p, p, p, p, None, spp, i(1), i(8), i(8), p, p, p, p) == INVALID
    for word, n_known in ((-33, 4), (36, 4), (32, 0), (2 ** 31 - 1, 4)):
        hits = np.zeros(4 * 1024, np.float32)
        hits[4 * 17] = np.array([word], np.int32).view(np.float32)[0]
        assert lib.adypt_probe_motion_gather(hits.ctypes.data_as(C.c_void_p), p, p, zero, i(1), i(8), i(8), p, C.c_int64(n_known), p, C.c_int64(4), i(5), p, p) == INVALID, word
    for n_known, n_records, tri_float4 in ((5, 4, 5), (-1, 4, 5), (2, 4, 4), (2, 4, 65)):
        assert lib.adypt_probe_motion_gather(p, p, p, zero, i(1), i(8), i(8), p, C.c_int64(n_known), p, C.c_int64(n_records), i(tri_float4), p, p) == INVALID
    for n, tri_float4 in ((0, 8), (-1, 8), (4, 4), ((1 << 20) + 1, 8)):
        assert lib.adypt_probe_motion_snapshot(p, i(tri_float4), C.c_int64(n), p) == INVALID
    for step in (0, -1, 65):
        assert lib.adypt_probe_atrous(p, p, p, p, i(8), i(8), i(step), C.c_float(4.0), C.c_float(0.1), i(0), p) == INVALID
    assert lib.adypt_probe_atrous(p, p, p, p, i(8), i(0), i(1), C.c_float(4.0), C.c_float(0.1), i(0), p) == INVALID and lib.adypt_probe_atrous(p, p, p, None, i(8), i(8), i(1), C.c_float(4.0), C.c_float(0.1), i(1), p) == INVALID
    for radius in (0, 4):
        assert lib.adypt_probe_rectify_window(i(radius), p, p, p, p, i(8), i(8), p, p, p) == INVALID
    assert lib.adypt_probe_rectify_window(i(3), p, p, p, p, i(8), i(8), None, p, p) == INVALID
    merge = lambda motion, rectify, xp, r0, kept, w=8: lib.adypt_probe_temporal_merge(i(motion), i(rectify), p, p, p, p, p, p, p, p, i(1), p, p, p, C.c_float(64.0), xp, xp, r0, r0,  # noqa: E731
                                                                                       C.c_float(1.0), i(w), i(8), p, p, p, kept)
    assert merge(1, 0, None, None, None) == INVALID and merge(0, 1, None, None, p) == INVALID and merge(0, 1, None, p, None) == INVALID and merge(0, 0, None, None, None, w=0) == INVALID
