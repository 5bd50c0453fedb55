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


KERNEL_ENTRIES = ("denoise_prepare", "atrous", "rectify_window", "temporal_merge", "motion_gather", "motion_snapshot", "temporal_merge_virtual", "denoise_prepare_instance",
                  "temporal_merge_moments", "moments_variance", "chain_start", "chain_step")


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


def test_the_moments_and_prepare_instance_entries_refuse_what_a_kernel_must_not_be_given():
    lib = P.lib()
    buf = np.zeros(4 * 1024, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    i = C.c_int
    spp = np.array([8], np.int32).ctypes.data_as(C.c_void_p)
    zero = np.array([0], np.int32).ctypes.data_as(C.c_void_p)
    prepare = lambda instance, b=zero, nb=1, w=8, h=8, x0=p, gv=p, xv=p: lib.adypt_probe_denoise_prepare_instance(i(instance), p, p, p, p, p, p, b, spp, i(nb), i(w), i(h), x0, p, p, p, gv, xv)  # noqa: E731
    assert prepare(-1) == INVALID and prepare(3) == INVALID, "an instance that is none of the three"
    assert prepare(2, gv=None) == INVALID and prepare(2, xv=None) == INVALID and prepare(0, x0=None) == INVALID and prepare(1, b=None) == INVALID
    for block, w, h in ((-1, 8, 8), (1, 8, 8), (2, 33, 9), (0, 0, 8), (0, 8, 4097)):
        b = np.array([block], np.int32).ctypes.data_as(C.c_void_p)
        for instance in (0, 1, 2):
            assert prepare(instance, b=b, w=w, h=h) == INVALID, (instance, block, w, h)
    assert prepare(0, nb=0) == INVALID
    merge = lambda motion, xp, w=8, h=8, x0=p, out=p: lib.adypt_probe_temporal_merge_moments(i(motion), x0, p, p, p, p, p, p, p, i(1), p, p, p, C.c_float(64.0), xp, xp, i(w), i(h), p, p, out)  # noqa: E731
    assert merge(1, None) == INVALID and merge(0, None, w=0) == INVALID and merge(0, None, h=4097) == INVALID and merge(0, None, x0=None) == INVALID and merge(0, p, out=None) == INVALID
    variance = lambda w=8, h=8, origin=p, count=p: lib.adypt_probe_moments_variance(p, p, p, p, i(w), i(h), origin, p, p, count)  # noqa: E731
    assert variance(w=0) == INVALID and variance(h=-1) == INVALID and variance(w=4097) == INVALID and variance(origin=None) == INVALID and variance(count=None) == INVALID


def test_the_chain_entries_refuse_what_a_kernel_must_not_be_given():
    """Null pointers, sizes out of range, and a hit word, a material id or a pixel word outside the slack: refused before anything is allocated or
    launched — a chain kernel reads where a hit word and a material id say and writes where a pixel word says."""
    lib = P.lib()
    i, u32, i64, f = C.c_int, C.c_uint32, C.c_int64, C.c_float
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    buf = np.zeros(8 * 1024, np.float32)
    p = ptr(buf)
    zero = ptr(np.array([0], np.int32))
    tris, mats = np.zeros((4, 32), np.float32), np.zeros((2, 20), np.float32)
    mats.view(np.int32)[:, 0] = -1
    tex = np.zeros((3, 4, 3), np.uint8)

    def start(tris=tris, n_tris=4, mats=mats, n_mats=2, tex=None, tw=0, th=0, hits=p, blocks=zero, nb=1, w=8, h=8, origin=p, bounces=8, segments=2, cap=512, state=p, counts=p):
        return lib.adypt_probe_chain_start(i(0), None if tris is None else ptr(tris), i64(n_tris), None if mats is None else ptr(mats), i(n_mats), None if tex is None else ptr(tex), i(tw),
                                           i(th), p, p, p, hits, blocks, i(nb), i(w), i(h), origin, f(0.001), i(bounces), i(segments), u32(cap), state, p, p, p, counts)

    def step(tris=tris, n_tris=4, mats=mats, n_mats=2, n_px=1024, segments=2, cap=8, in_d=p, in_hit=p, bounces=8, unfold=0, virt=p, origin=p, out_count=p):
        return lib.adypt_probe_chain_step(i(unfold), ptr(tris), i64(n_tris), ptr(mats), i(n_mats), None, i(0), i(0), p, p, p, p, i(n_px), i(segments), u32(cap), p, in_d, in_hit, p,
                                          i(bounces), f(0.001), p, p, p, out_count, p, virt, origin)
    for call in (start, step):
        assert call(n_tris=0) == INVALID and call(n_tris=(1 << 20) + 1) == INVALID and call(n_mats=0) == INVALID and call(n_mats=4097) == INVALID
        assert call(bounces=0) == INVALID and call(bounces=9) == INVALID and call(segments=0) == INVALID and call(segments=65) == INVALID and call(cap=0) == INVALID and call(cap=(1 << 20) + 1) == INVALID
        for matid in (-33, 34):  # (a triangle's material id farther than 32 from [0, n_mats))
            bad = tris.copy()
            bad.view(np.int32)[2, 18] = matid
            assert call(tris=bad) == INVALID, matid
    assert start(tris=None) == INVALID and start(mats=None) == INVALID and start(hits=None) == INVALID and start(origin=None) == INVALID and start(state=None) == INVALID and start(counts=None) == INVALID
    assert start(blocks=None) == INVALID and start(nb=0) == INVALID and start(nb=65) == INVALID and start(w=0) == INVALID and start(h=4097) == INVALID
    assert start(blocks=ptr(np.array([1], np.int32))) == INVALID, "a block outside the picture's grid"
    assert start(tex=tex, tw=0, th=3) == INVALID and start(tex=tex, tw=4, th=-1) == INVALID
    named = mats.copy()
    named.view(np.int32)[1, 0] = 0  # names the texture, and describes it as (0, 0, 0)
    assert start(mats=named, tex=tex, tw=4, th=3) == INVALID, "a material that names the texture and does not describe it"
    for word in (-33, 4 + 32, 2 ** 31 - 2, -2 ** 31):
        hits = np.zeros(4 * 1024, np.float32)
        hits.view(np.int32)[4 * 17] = word
        assert start(hits=ptr(hits)) == INVALID, word
        queue = np.zeros(4 * 16, np.float32)
        queue.view(np.int32)[4 * 5] = word
        assert step(in_hit=ptr(queue)) == INVALID, word
    for word in (-33, 1024 + 32, 2 ** 31 - 2, -2 ** 31):
        queue = np.zeros(4 * 16, np.float32)
        queue.view(np.int32)[4 * 5 + 3] = word
        assert step(in_d=ptr(queue)) == INVALID, word
    assert step(n_px=0) == INVALID and step(n_px=(1 << 22) + 1) == INVALID and step(in_d=None) == INVALID and step(out_count=None) == INVALID
    assert step(unfold=1, virt=None) == INVALID and step(unfold=1, origin=None) == INVALID
