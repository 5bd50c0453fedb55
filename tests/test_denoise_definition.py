"""The denoiser's definition (csrc/device/denoise.hpp) compiled on the host and held bit for bit against its numpy float32 restatement
(tests/denoise_truth.py): on inputs the CPU oracle makes, and on hand-made edge cases.  Its quality is measured against the oracle's converged
image, never against the code under test.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import denoise_truth as D
from tests import noise_truth as T
from tests.helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
SEED = 31

DRIVER = r"""
#include "denoise.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace adypt;
// IN:  int32 w, h, levels; float32 sigma_l, sigma_z; float32 C[h][w][3], m2[h][w], n[h][w], A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
// OUT: float32 rgb[h][w][3]
struct Img {
	const Dn4 *a, *b, *c;
	Dn4 x0(int i) const { return a[i]; }
	Dn4 x1(int i) const { return b[i]; }
	Dn4 x2(int i) const { return c[i]; }
};
int main(int argc, char **argv)
{
	if(argc != 3) return 2;
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if(!in || !out) return 3;
	int32_t h[3]; float s[2];
	if(fread(h, 4, 3, in) != 3 || fread(s, 4, 2, in) != 2) return 4;
	const int width = h[0], height = h[1];
	const size_t n = (size_t)width * height;
	std::vector<float> C(n * 3), m2(n), cnt(n), A(n * 3), N(n * 3), P(n * 3);
	std::vector<uint8_t> hit(n);
	if(fread(C.data(), 4, n * 3, in) != n * 3 || fread(m2.data(), 4, n, in) != n || fread(cnt.data(), 4, n, in) != n || fread(A.data(), 4, n * 3, in) != n * 3 ||
	   fread(N.data(), 4, n * 3, in) != n * 3 || fread(P.data(), 4, n * 3, in) != n * 3 || fread(hit.data(), 1, n, in) != n) return 4;
	const DenoiseParams prm{h[2], s[0], s[1]};
	if(!denoise_params_valid(prm)) return 5;
	std::vector<Dn4> x0(n), x0b(n), x1(n), x2(n), xa(n);
	for(size_t i = 0; i < n; ++i)
	{
		x0[i] = denoise_prepare(C[3 * i], C[3 * i + 1], C[3 * i + 2], m2[i], cnt[i], A[3 * i], A[3 * i + 1], A[3 * i + 2]);
		x1[i] = Dn4{N[3 * i], N[3 * i + 1], N[3 * i + 2], hit[i] ? 1.0f : 0.0f};
		x2[i] = Dn4{P[3 * i], P[3 * i + 1], P[3 * i + 2], 0.0f};
		xa[i] = Dn4{A[3 * i], A[3 * i + 1], A[3 * i + 2], 0.0f};
	}
	for(int l = 0; l < prm.levels; ++l)
	{
		const Img img{x0.data(), x1.data(), x2.data()};
		for(int y = 0; y < height; ++y)
			for(int x = 0; x < width; ++x) x0b[(size_t)y * width + x] = denoise_level(img, width, height, x, y, 1 << l, prm.sigma_l, prm.sigma_z);
		x0.swap(x0b);
	}
	std::vector<float> rgb(n * 3);
	for(size_t i = 0; i < n; ++i) denoise_remodulate(x0[i], xa[i], &rgb[3 * i]);
	fwrite(rgb.data(), 4, rgb.size(), out);
	fclose(out);
	return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("denoise_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", DEVICE, src, "-o", exe])
    return exe, str(d)


def run_driver(driver, C, m2, n, A, N, P, hit, levels=5, sigma_l=4.0, sigma_z=0.1):
    exe, d = driver
    h, w = np.shape(m2)
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([w, h, levels], np.int32).tobytes() + np.array([sigma_l, sigma_z], np.float32).tobytes())
        for a in (C, m2, n, A, N, P):
            f.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
        f.write(np.ascontiguousarray(hit).astype(np.uint8).tobytes())
    subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    return np.fromfile(os.path.join(d, "out.bin"), dtype=np.float32).reshape(h, w, 3)


def check(driver, inputs, **kw):
    got = run_driver(driver, *inputs, **kw)
    want = D.denoise(*inputs, **kw)
    differing = int((bits(got) != bits(want)).sum())
    assert differing == 0, "%d words differ from the numpy restatement (%s)" % (differing, kw)
    return got


def test_header_needs_no_hip_include_and_has_no_fma_exp_or_pow():
    text = open(os.path.join(DEVICE, "denoise.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in "".join(l for l in code.splitlines() if l.startswith("#include")).lower()
    assert not re.search(r"\b(fmaf?|expf?|exp2f?|powf?|__builtin\w*)\b", code)
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", DEVICE, "-x", "c++", "-"],
                   input=b'#include "denoise.hpp"\nint main() { return adypt::denoise_params_valid(adypt::kDenoiseDefaults) ? 0 : 1; }\n', check=True)


def oracle_inputs(scene_cache, sobol_matrices, name, w, h, life, sub, spp, want_samples=True):
    """(inputs of the filter after spp frames, oracle scene, oracle parameters, shift image), everything made by the CPU oracle."""
    from adypt_amd import api, scenes
    spec = scenes.make_scene(name, scene_cache, width=w, height=h, pt={"tmpLifetime": life, "maxBounce": 6, "subpixel": sub})
    cfg = api.InstanceConfig()
    assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
    sc = api.Scene()
    assert sc.LoadFromFile(cfg.m_obj_filename)
    b = api.WideBVH()
    if not b.LoadFromFile(cfg.m_bvh_filename, cfg.bvh_params()):
        b.Build(sc, cfg.bvh_params())
        assert b.SaveToFile(cfg.m_bvh_filename, cfg.bvh_params())
    osc = O.Scene(b.nodes, b.tri_indices, sc.triangles, sc.materials, textures=sc.textures)
    P, shift = T.oracle_params(cfg.c), O.shift_bytes(SEED, w, h)
    samples = T.frame_samples(osc, P, shift, sobol_matrices, spp)
    _, m2 = T.moments(samples)
    state = O.PathTracerState(w, h)
    O.pt_frames(osc, P, shift, sobol_matrices, state, spp)
    guides = [O.primary_frame(osc, P, t) for t in (0, 4, 5)]
    hit = guides[0][1]["tri_id"] != -1
    inputs = (state.accum[..., :3].copy(), m2, spp, guides[0][0][..., :3].copy(), guides[1][0][..., :3].copy(), guides[2][0][..., :3].copy(), hit)
    return inputs, osc, P, shift, state


def converged(osc, P, shift, sobol_matrices, state, spp):
    O.pt_frames(osc, P, shift, sobol_matrices, state, spp - state.spp)
    return state.accum[..., :3].copy()


def test_definition_on_oracle_inputs_and_quality_tiny0(driver, scene_cache, sobol_matrices):
    """tiny0 100x75, 16 spp: the header against numpy at 1, 5 and 6 levels (at 6 most taps lie outside a 100-pixel-wide image); the default filter
    against the oracle's 2048-spp image."""
    inputs, osc, P, shift, state = oracle_inputs(scene_cache, sobol_matrices, "tiny0", 100, 75, 16, 3, 16)
    assert inputs[6].any() and not inputs[6].all()  # hits and sky
    out = {levels: check(driver, inputs, levels=levels) for levels in (1, 5, 6)}
    check(driver, inputs, levels=3, sigma_l=1.5, sigma_z=0.5)
    for levels, img in out.items():
        assert np.isfinite(img).all(), "levels %d" % levels
    ref = converged(osc, P, shift, sobol_matrices, state, 2048)
    raw, den = D.rmse(inputs[0], ref), D.rmse(out[5], ref)
    print("tiny0 100x75 16 spp against 2048 spp: rmse raw %.4f denoised %.4f ratio %.3f" % (raw, den, den / raw))
    assert den / raw < 0.9


def test_quality_sibenik(scene_cache, sobol_matrices):
    """sibenik 96x54, 20 spp, tmpLifetime 3, subpixel 1, maxBounce 6, defaults: the filtered image is at most half as far from the oracle's
    1024-spp image as the raw one."""
    inputs, osc, P, shift, state = oracle_inputs(scene_cache, sobol_matrices, "sibenik", 96, 54, 3, 1, 20)
    den = D.denoise(*inputs)
    assert np.isfinite(den).all()
    ref = converged(osc, P, shift, sobol_matrices, state, 1024)
    raw, got = D.rmse(inputs[0], ref), D.rmse(den, ref)
    print("sibenik 96x54 20 spp against 1024 spp: rmse raw %.4f denoised %.4f ratio %.3f" % (raw, got, got / raw))
    assert got <= 0.5 * raw


def plane(h, w, rs, hit=True, var=True):
    """A plane z = 0 seen head-on: unit normals, positions on a grid, random radiance and moments."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    C = rs.uniform(0, 2, size=(h, w, 3)).astype(np.float32)
    m2 = (rs.uniform(0, 3, size=(h, w)).astype(np.float32) if var else np.zeros((h, w), np.float32))
    A = rs.uniform(0.1, 0.9, size=(h, w, 3)).astype(np.float32)
    N = np.zeros((h, w, 3), np.float32); N[..., 2] = 1
    P = np.stack([xx * np.float32(0.1), yy * np.float32(0.1), np.zeros_like(xx)], -1)
    hitm = np.full((h, w), hit, bool)
    if not hit:
        A[:] = 0; N[:] = 0; P[:] = 0
    return [C, m2, 8, A, N, P, hitm]


def test_definition_on_edge_cases(driver):
    rs = np.random.RandomState(7)
    for levels in (1, 5, 6):
        # the smallest images: every tap but the centre lies outside, or nearly
        for h, w in ((1, 1), (2, 3)):
            out = check(driver, plane(h, w, rs), levels=levels)
            assert np.isfinite(out).all()
        # nothing but sky
        out = check(driver, plane(9, 13, rs, hit=False), levels=levels)
        assert np.isfinite(out).all()
        # zero variance: sl is the floor 1e-4, the luminance weight all but closes
        inp = plane(9, 13, rs, var=False)
        out = check(driver, inp, levels=levels)
        assert np.isfinite(out).all()
    # hit pixels of albedo 0 (the floor 0.01 keeps the division finite), a miss among them
    inp = plane(10, 12, rs)
    inp[3][2:6, 3:9] = 0
    inp[6][4, 4] = False
    assert np.isfinite(check(driver, inp)).all()
    # a hit pixel whose eight neighbours are all misses, and a miss whose neighbours are all hits
    inp = plane(11, 11, rs)
    inp[6][4:7, 4:7] = False
    inp[6][5, 5] = True
    inp[6][9, 2] = False
    out = check(driver, inp)
    assert np.isfinite(out).all()
    # a NaN normal at a centre (every off-centre weight 0: the pixel keeps its own value) and so at its neighbours' taps
    inp = plane(12, 12, rs)
    inp[4][6, 6] = np.nan
    inp[4][0, 0, 1] = np.nan
    for levels in (1, 5):
        out = check(driver, inp, levels=levels)
        assert np.isfinite(out).all()
    got1 = check(driver, inp, levels=1)
    assert np.allclose(got1[6, 6], inp[0][6, 6], rtol=1e-6)
    # sample counts that differ per block, over partial blocks on both edges
    inp = plane(40, 70, rs)
    inp[2] = np.array([2, 8, 3, 17, 5, 64], np.int32)
    check(driver, inp)
    check(driver, inp, levels=6, sigma_l=0.5, sigma_z=2.0)


def test_the_new_symbols_are_declared_and_bound():
    from adypt_amd import _native as N
    header = open(os.path.join(ROOT, "include", "adypt_hip.h")).read()
    for name in ("adypt_denoise", "adypt_read_denoised", "adypt_read_denoise_guides", "adypt_multi_denoise", "adypt_multi_read_denoised", "adypt_multi_read_denoise_guides"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in N.EXPORTS and hasattr(N.lib, name), name
    assert "typedef struct adypt_denoise_params" in header and N.lib.adypt_abi_version() == 4
    import ctypes
    assert ctypes.sizeof(N.DenoiseParams) == 12


def test_the_named_edge_inputs(driver):
    """tests/denoise_edge_inputs.py's entries for prepare and the levels — the sizes round the 32 x 8 workgroup, sample counts 2 and 64 in neighbouring
    blocks, m2 = 0, albedo 0, Inf and NaN in the accumulator — at six levels (steps 1 .. 32) under both pairs of sigmas: zero differing words."""
    from tests import denoise_edge_inputs as E  # (here: the module imports this file's generators)
    for name, case in E.filter_cases().items():
        assert case["reach"](), name + ": the case does not reach what it is named after"
        for sigma_l, sigma_z in E.SIGMAS:
            kw = dict(levels=6, sigma_l=sigma_l, sigma_z=sigma_z)
            try:
                if np.isfinite(case["call"][0]).all() and np.isfinite(case["call"][1]).all():
                    check(driver, case["call"], **kw)
                else:
                    # radiance that is no number spreads through the levels as NaN, whose sign and payload the definition does not say (g++ and numpy
                    # order the operands of a product differently): NaN in the same places, equal words everywhere else
                    got, want = run_driver(driver, *case["call"], **kw), D.denoise(*case["call"], **kw)
                    assert np.isnan(want).any() and np.array_equal(np.isnan(got), np.isnan(want)), "NaN in other places than the numpy restatement"
                    assert int((bits(got) != bits(want))[~np.isnan(want)].sum()) == 0, "words differ from the numpy restatement (%s)" % kw
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e))
