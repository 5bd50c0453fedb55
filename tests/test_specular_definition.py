"""The chain through mirrors and glass (csrc/device/guide_chain.hpp) compiled on the host and held bit for bit against its numpy float32 restatement
(tests/specular_truth.py): whole chains over the CPU oracle's primary frames and closest hits, and hand-made steps.  The quality of the followed
guides is measured against the oracle's converged image, never against the code under test.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import denoise_truth as D
from tests import specular_truth as S
from tests import test_denoise_definition as DD  # its oracle inputs
from tests.helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
F = np.float32

DRIVER = r"""
#include "guide_chain.hpp"
#include <cstdint>
using namespace adypt;
static Ch3 ld(const float *a, int i) { return Ch3{a[3 * i], a[3 * i + 1], a[3 * i + 2]}; }
static void st(float *a, int i, const Ch3 &v) { a[3 * i] = v.x; a[3 * i + 1] = v.y; a[3 * i + 2] = v.z; }
extern "C" {
// chains i = 0 .. n-1 stand on a surface: T, d are updated where the chain goes on; albedo: of a chain that ends here
void sp_at_surface(int n, float *T, float *d, const int32_t *L, const uint8_t *bad, const int32_t *illum, const float *kd, const float *ks, const float *ior, const float *nrm, int K,
                   uint8_t *go, float *albedo)
{
	for(int i = 0; i < n; ++i)
	{
		ChainState s{ld(T, i), ld(d, i), L[i]};
		const ChainMaterial m{bad[i] != 0, illum[i], ld(kd, i), ld(ks, i), ior[i]};
		ChainEnd end;
		go[i] = chain_at_surface(s, m, ld(nrm, i), Ch3{0.0f, 0.0f, 0.0f}, K, &end) == kChainGoesOn ? 1 : 0;
		st(albedo, i, end.albedo);
		if(go[i]) { st(T, i, s.t); st(d, i, s.d); }
	}
}
void sp_at_primary(int n, const uint8_t *bad, const int32_t *illum, const float *ks, const float *ior, const float *nrm, const float *p, const float *origin, int K, uint8_t *go, float *d,
                   float *T)
{
	for(int i = 0; i < n; ++i)
	{
		ChainState s;
		const ChainMaterial m{bad[i] != 0, illum[i], Ch3{0.0f, 0.0f, 0.0f}, ld(ks, i), ior[i]};
		go[i] = chain_at_primary(s, m, ld(nrm, i), ld(p, i), origin, K) == kChainGoesOn ? 1 : 0;
		st(d, i, go[i] ? s.d : Ch3{0.0f, 0.0f, 0.0f});
		st(T, i, go[i] ? s.t : Ch3{1.0f, 1.0f, 1.0f});
	}
}
void sp_hit_point(int n, const float *tri, const float *u, const float *v, float *p, float *nrm)
{
	for(int i = 0; i < n; ++i)
	{
		Ch3 a, b;
		chain_hit_point(tri + 18 * i, u[i], v[i], &a, &b);
		st(p, i, a); st(nrm, i, b);
	}
}
void sp_mirror(int n, const float *d, const float *nrm, float *out) { for(int i = 0; i < n; ++i) st(out, i, chain_mirror(ld(d, i), ld(nrm, i))); }
void sp_dielectric(int n, const float *d, const float *nrm, const float *ior, float *out, uint8_t *refracted)
{
	for(int i = 0; i < n; ++i) { bool r; st(out, i, chain_dielectric(ld(d, i), ld(nrm, i), ior[i], &r)); refracted[i] = r ? 1 : 0; }
}
int sp_escaped_class(int length) { ChainState s{Ch3{1, 1, 1}, Ch3{0, 0, 1}, length}; return chain_escaped(s).cls; }
}
"""


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class HeaderOps:
    """specular_truth.NumpyOps' operations through the compiled header."""

    def __init__(self, lib):
        self.lib = lib

    def at_surface(self, T, d, L, bad, illum, kd, ks, ior, n, K):
        cnt = len(L)
        T, d, kd, ks, ior, n = f32(T).copy(), f32(d).copy(), f32(kd), f32(ks), f32(ior), f32(n)
        L, illum, bad8 = np.ascontiguousarray(L, np.int32), np.ascontiguousarray(illum, np.int32), np.ascontiguousarray(bad).astype(np.uint8)
        go, albedo = np.zeros(cnt, np.uint8), np.zeros((cnt, 3), np.float32)
        self.lib.sp_at_surface(cnt, ptr(T), ptr(d), ptr(L), ptr(bad8), ptr(illum), ptr(kd), ptr(ks), ptr(ior), ptr(n), int(K), ptr(go), ptr(albedo))
        return go.astype(bool), albedo, d, T

    def at_primary(self, bad, illum, ks, ior, n, p, origin, K):
        cnt = len(illum)
        ks, ior, n, p, origin = f32(ks), f32(ior), f32(n), f32(p), f32(origin)
        illum, bad8 = np.ascontiguousarray(illum, np.int32), np.ascontiguousarray(bad).astype(np.uint8)
        go, d, T = np.zeros(cnt, np.uint8), np.zeros((cnt, 3), np.float32), np.zeros((cnt, 3), np.float32)
        self.lib.sp_at_primary(cnt, ptr(bad8), ptr(illum), ptr(ks), ptr(ior), ptr(n), ptr(p), ptr(origin), int(K), ptr(go), ptr(d), ptr(T))
        return go.astype(bool), d, T

    def hit_point(self, tri, u, v):
        tri, u, v = f32(tri), f32(u), f32(v)
        p, n = np.zeros((len(u), 3), np.float32), np.zeros((len(u), 3), np.float32)
        self.lib.sp_hit_point(len(u), ptr(tri), ptr(u), ptr(v), ptr(p), ptr(n))
        return p, n

    def mirror(self, d, n):
        d, n = f32(d), f32(n)
        out = np.zeros_like(d)
        self.lib.sp_mirror(len(d), ptr(d), ptr(n), ptr(out))
        return out

    def dielectric(self, d, n, ior):
        d, n, ior = f32(d), f32(n), f32(ior)
        out, r = np.zeros_like(d), np.zeros(len(d), np.uint8)
        self.lib.sp_dielectric(len(d), ptr(d), ptr(n), ptr(ior), ptr(out), ptr(r))
        return out, r.astype(bool)


def build_header(d):
    """HeaderOps over the driver compiled in the directory d"""
    src, so = str(d / "driver.cpp"), str(d / "libdriver.so")
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", DEVICE, src, "-o", so])
    return HeaderOps(C.CDLL(so))


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    return build_header(tmp_path_factory.mktemp("specular_driver"))


def test_header_needs_no_hip_include_and_has_no_fma_exp_or_pow():
    text = open(os.path.join(DEVICE, "guide_chain.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in "".join(l for l in code.splitlines() if l.startswith("#include")).lower()
    assert not re.search(r"\b(fmaf?|expf?|exp2f?|powf?|__builtin\w*)\b", code)
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", DEVICE, "-x", "c++", "-"],
                   input=b'#include "guide_chain.hpp"\nint main() { return adypt::chain_bounces_valid(8) && !adypt::chain_bounces_valid(9) && !adypt::chain_bounces_valid(0) ? 0 : 1; }\n', check=True)


def assert_same_chain(got, want, tag):
    for k in ("albedo", "normal", "position"):
        differing = int((bits(got[k]) != bits(want[k])).sum())
        assert differing == 0, "%s: %d words of %s differ from the numpy restatement" % (tag, differing, k)
    assert np.array_equal(got["chain"], want["chain"]), tag + ": classes"
    for k in ("rays", "followed", "escaped", "truncated"):
        assert got[k] == want[k], "%s: %s" % (tag, k)


_inputs = {}


def inputs_of(scene_cache, sobol_matrices, name, w, h, life, sub, spp):
    key = (name, w, h, life, sub, spp)
    if key not in _inputs:
        _inputs[key] = DD.oracle_inputs(scene_cache, sobol_matrices, name, w, h, life, sub, spp)
    return _inputs[key]


def test_whole_chains_tiny0(header, scene_cache, sobol_matrices):
    """tiny0 100x75 at K = 1, 2, 8: the header against numpy, zero differing words; the scene reaches every kind of end."""
    inputs, osc, P, shift, state = inputs_of(scene_cache, sobol_matrices, "tiny0", 100, 75, 3, 1, 16)
    primary = S.primary_guides(osc, P)
    for K in (1, 2, 8):
        want = S.chain_guides(osc, P, K, primary)
        assert_same_chain(S.chain_guides(osc, P, K, primary, ops=header), want, "tiny0 K = %d" % K)
        c = want["chain"]
        assert (c == 0).any() and (c == 1).any() and (c < 0).any() and (c > 1).any(), "K = %d: sky, plain hits, escaped and followed pixels" % K
        if K < 8:
            assert want["truncated"] > 0
    c = S.chain_guides(osc, P, 8, primary)["chain"]
    assert (c >= 4).any() or (c <= -4).any(), "a chain of three bounces or more"
    # followed pixels have the guides of another surface; the others keep the primary capture's
    same = c <= 1
    want8 = S.chain_guides(osc, P, 8, primary)
    for k in ("albedo", "normal", "position"):
        assert np.array_equal(bits(want8[k][same & (c >= 0)]), bits(primary[k][same & (c >= 0)])), k


def test_whole_chains_sibenik(header, scene_cache, sobol_matrices):
    inputs, osc, P, shift, state = inputs_of(scene_cache, sobol_matrices, "sibenik", 96, 54, 3, 1, 20)
    primary = S.primary_guides(osc, P)
    want = S.chain_guides(osc, P, 4, primary)
    assert want["followed"] > 0
    assert_same_chain(S.chain_guides(osc, P, 4, primary, ops=header), want, "sibenik K = 4")


def same_words(a, b):
    return np.array_equal(bits(f32(a)), bits(f32(b)))


def test_hand_made_steps(header):
    """each step is asserted to reach what it is named after, then the header's words are the numpy restatement's"""
    N = S.NumpyOps()
    up = f32([[0, 1, 0]])
    # grazing incidence: d . n = 0 — the mirror leaves the direction, the dielectric takes the entering branch with cosi = 0
    d = f32([[1, 0, 0]])
    assert S.dot(d, up)[0] == 0
    assert same_words(header.mirror(d, up), S.mirror(d, up)) and same_words(header.mirror(d, up), d)
    got, want = header.dielectric(d, up, f32([1.5])), S.dielectric(d, up, f32([1.5]))
    assert same_words(got[0], want[0]) and got[1][0] == want[1][0] and np.isfinite(got[0]).all()
    # total internal reflection: leaving glass (d . n > 0) at a shallow angle
    d = S.normalize(f32([[1, 0.2, 0]]))[0]
    got, want = header.dielectric(d, up, f32([1.5])), S.dielectric(d, up, f32([1.5]))
    assert S.dot(d, up)[0] > 0 and not got[1][0] and not want[1][0], "no refraction"
    assert same_words(got[0], want[0]) and same_words(got[0], S.reflect(d, up))
    # a ray entering and a ray leaving glass: both refracted, unit length
    for d in (f32([[0.6, -0.8, 0]]), S.normalize(f32([[0.1, 1, 0]]))[0]):
        got, want = header.dielectric(d, up, f32([1.5])), S.dielectric(d, up, f32([1.5]))
        assert got[1][0] and want[1][0], "refraction"
        assert same_words(got[0], want[0]) and abs(float(S.dot(got[0], got[0])[0]) - 1) < 1e-6 and got[0][0, 1] * d[0, 1] > 0
    # a mirror normal that faces away from the ray is flipped first
    d = f32([[0.6, 0.8, 0]])
    assert S.dot(d, up)[0] > 0
    assert same_words(header.mirror(d, up), S.mirror(d, up)) and same_words(header.mirror(d, up), header.mirror(d, -up)) and header.mirror(d, up)[0, 1] < 0
    # an interpolated normal of length zero: the normal is (0, 0, 0), a mirror there lets the ray go straight on
    tri = f32([[0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0, -1, 0, 0, 0, 0, 0]])
    u, v = f32([0.5]), f32([0.5])
    p, n = header.hit_point(tri, u, v)
    pw, nw = S.hit_point(tri, u, v)
    assert same_words(p, pw) and same_words(n, nw) and not n.any(), "a zero normal"
    d = S.normalize(f32([[1, 2, 3]]))[0]
    args = (np.ones((1, 3), np.float32), d, np.array([1], np.int32), np.array([False]), np.array([3], np.int32), f32([[0, 0, 0]]), f32([[0.5, 0.6, 0.7]]), f32([1.0]), n, 8)
    got, want = header.at_surface(*args), N.at_surface(*args)
    assert got[0][0] and want[0][0] and same_words(got[2], d) and all(same_words(a, b) for a, b in zip(got[1:], want[1:]))
    # a NaN normal never reaches a traced direction: the chain ends there
    args_nan = args[:8] + (f32([[np.nan, 0, 0]]), 8)
    assert not header.at_surface(*args_nan)[0][0] and not N.at_surface(*args_nan)[0][0]
    # truncation exactly at K = 1: a mirror met after one bounce ends the chain with albedo T x Ks
    T = f32([[0.5, 0.25, 1.0]])
    args = (T, d, np.array([1], np.int32), np.array([False]), np.array([3], np.int32), f32([[0.9, 0.9, 0.9]]), f32([[0.5, 0.6, 0.7]]), f32([1.0]), up, 1)
    got, want = header.at_surface(*args), N.at_surface(*args)
    assert not got[0][0] and not want[0][0] and same_words(got[1], want[1]) and same_words(got[1], T * f32([[0.5, 0.6, 0.7]]))
    assert header.at_surface(*(args[:9] + (2,)))[0][0], "the same surface goes on at K = 2"
    # glass cut at K keeps the throughput; a glossy lobe (illum 2) and a bad material end the chain as diffuse surfaces do
    args = (T, d, np.array([1], np.int32), np.array([False]), np.array([7], np.int32), f32([[0.9, 0.9, 0.9]]), f32([[0.5, 0.6, 0.7]]), f32([1.5]), up, 1)
    assert same_words(header.at_surface(*args)[1], T) and same_words(N.at_surface(*args)[1], T)
    for bad, illum in ((False, 2), (True, 0)):
        kd = f32([[0, 0, 0]]) if bad else f32([[0.9, 0.8, 0.7]])
        args = (T, d, np.array([1], np.int32), np.array([bad]), np.array([illum], np.int32), kd, f32([[0.5, 0.6, 0.7]]), f32([1.5]), up, 8)
        got, want = header.at_surface(*args), N.at_surface(*args)
        assert not got[0][0] and not want[0][0] and same_words(got[1], want[1]) and same_words(got[1], T * kd)
    assert header.lib.sp_escaped_class(0) == -1 and header.lib.sp_escaped_class(3) == -4


def test_classes_0_and_1_through_the_class_aware_level_are_the_plain_filter(scene_cache, sobol_matrices):
    inputs, osc, P, shift, state = inputs_of(scene_cache, sobol_matrices, "tiny0", 100, 75, 3, 1, 16)
    hit = inputs[6]
    assert hit.any() and not hit.all()
    assert np.array_equal(bits(S.denoise(*inputs[:6], hit.astype(np.int8))), bits(D.denoise(*inputs)))


def quality(scene_cache, sobol_matrices, name, w, h, life, sub, spp, ref_spp, K=8):
    inputs, osc, P, shift, state = inputs_of(scene_cache, sobol_matrices, name, w, h, life, sub, spp)
    g = S.chain_guides(osc, P, K)
    plain = D.denoise(*inputs)
    followed = S.denoise(inputs[0], inputs[1], inputs[2], g["albedo"], g["normal"], g["position"], g["chain"])
    ref = DD.converged(osc, P, shift, sobol_matrices, state, ref_spp)
    chain_px = g["chain"] != inputs[6].astype(np.int8)  # the primary hit is a delta material
    assert chain_px.any()
    fig = dict(all=(D.rmse(plain, ref), D.rmse(followed, ref)), chain=(D.rmse(plain[chain_px], ref[chain_px]), D.rmse(followed[chain_px], ref[chain_px])),
               other=(D.rmse(plain[~chain_px], ref[~chain_px]), D.rmse(followed[~chain_px], ref[~chain_px])))
    print("%s %dx%d %d spp against %d spp, K = %d, %d chain px: rmse plain -> followed: all %.4f -> %.4f, chain px %.4f -> %.4f, other px %.4f -> %.4f"
          % ((name, w, h, spp, ref_spp, K, int(chain_px.sum())) + fig["all"] + fig["chain"] + fig["other"]))
    return fig


def test_quality_tiny0(scene_cache, sobol_matrices):
    """tiny0 100x75, 16 spp (tmpLifetime 3, subpixel 1) against 2048 spp: the order only"""
    fig = quality(scene_cache, sobol_matrices, "tiny0", 100, 75, 3, 1, 16, 2048)
    assert fig["all"][1] <= fig["all"][0] and fig["chain"][1] < fig["chain"][0]


def test_quality_sibenik(scene_cache, sobol_matrices):
    """sibenik 192x108, 20 spp (tmpLifetime 3, subpixel 1) against 1024 spp: the order only"""
    fig = quality(scene_cache, sobol_matrices, "sibenik", 192, 108, 3, 1, 20, 1024)
    assert fig["all"][1] <= fig["all"][0] and fig["chain"][1] < fig["chain"][0]


def test_the_new_symbols_are_declared_and_bound():
    from adypt_amd import _native as N
    header = open(os.path.join(ROOT, "include", "adypt_hip.h")).read()
    for name in ("adypt_denoise_specular", "adypt_read_denoise_guides_specular", "adypt_get_denoise_specular", "adypt_multi_denoise_specular",
                 "adypt_multi_read_denoise_guides_specular", "adypt_multi_get_denoise_specular"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in N.EXPORTS and hasattr(N.lib, name), name
    assert "typedef struct adypt_specular_params" in header and N.lib.adypt_abi_version() == 4
    assert C.sizeof(N.SpecularParams) == 4 and C.sizeof(N.DenoiseSpecular) == 56


def assert_same_arrays(got, want, keys, tag):
    for k in keys:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        differing = int((bits(a) != bits(b)).sum()) if a.dtype == np.float32 else int((a != b).sum())
        assert differing == 0, "%s: %d words of %s differ from the numpy restatement" % (tag, differing, k)


def test_the_probes_edge_inputs_through_the_header(header):
    """tests/chain_edge_inputs.py — what tests/test_gpu_chain_probes.py gives k_chain_start<false> and k_chain_step<false> — with chain_at_primary,
    chain_hit_point and chain_at_surface of the compiled header in place of numpy's: the same followed pixels, states, rays, guides and counts to the bit,
    and every case reaches what it is named after.  The GPU run then adds only kernel against truth."""
    from tests import chain_edge_inputs as CE
    sc = CE.scene()
    for picture in CE.START_PICTURES:
        for n_blocks in (1, 2, 3):
            for pattern in CE.START_PATTERNS:
                case = CE.start_case(picture, n_blocks, pattern)
                want = CE.start_truth(sc, case, False)
                assert CE.start_reach(case, want), (picture, n_blocks, pattern)
                assert_same_arrays(CE.start_truth(sc, case, False, ops=header), want, ("go", "hits_w", "state", "o", "d"), "start %s %d %s" % (picture, n_blocks, pattern))
    case = CE.overflow_case()
    want = CE.start_truth(sc, case, False)
    assert CE.start_reach(case, want) and want["go"][:64].all() and want["go"].sum() == 64
    assert_same_arrays(CE.start_truth(sc, case, False, ops=header), want, ("go", "hits_w", "state", "o", "d"), "start overflow")
    for name in CE.STEP_COUNTS:
        case = CE.step_case(name)
        want = CE.step_truth(sc, case, False)
        assert CE.step_reach(sc, case, want, False), name
        got = CE.step_truth(sc, case, False, ops=header)
        assert_same_arrays(got, want, ("albedo", "normal", "position", "hits", "state", "go"), "step " + name)
        assert_same_arrays(dict(o=got["rays"][0], d=got["rays"][1]), dict(o=want["rays"][0], d=want["rays"][1]), ("o", "d"), "step %s: the rays" % name)
        assert (got["escaped"], got["truncated"]) == (want["escaped"], want["truncated"])
