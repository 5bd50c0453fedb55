"""Rectifying stale history: the definition (csrc/device/rectify.hpp and the rectified merge of csrc/device/temporal.hpp) compiled on the host and held
bit for bit against its numpy float32 restatement (tests/rectify_truth.py): on the camera sequences of tests/test_temporal_definition.py, the last
pose under the config's sun and under a quarter and four times of it, and on hand-made edge cases.  Its quality is measured against the oracle's
converged image of the last pose, never against the code under test.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import denoise_truth as D
from tests import noise_truth as T
from tests import rectify_truth as RT
from tests import temporal_truth as TT
from tests import test_temporal_definition as TD  # its camera sequences, its hand-made walls and its word count

ROOT = TD.ROOT
DEVICE = TD.DEVICE
SEED = TD.SEED
F = np.float32
differing = TD.differing

DRIVER = r"""
#include "temporal.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace adypt;
// IN:  int32 w, h, levels, have, rectify, radius; float32 sigma_l, sigma_z, cap, gamma, origin[3] (of the call's camera);
//      the call:    float32 C[h][w][3], m2[h][w], n[h][w], A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
//      the history: float32 origin[3], inv_proj[16], inv_view[16], D[h][w][3], V[h][w], n[h][w], A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
// OUT: float32 Dm[h][w][3], Vm[h][w], n_out[h][w], kept[h][w], R0[h][w][4], R1[h][w][4], rgb[h][w][3]
struct Img {
	const Dn4 *a, *b, *c, *d;
	Dn4 x0(int i) const { return a[i]; }
	Dn4 x1(int i) const { return b[i]; }
	Dn4 x2(int i) const { return c[i]; }
	Dn4 xa(int i) const { return d[i]; }
};
struct Hist {
	const Dn4 *a, *b, *c, *d;
	Dn4 h0(int i) const { return a[i]; }
	Dn4 h1(int i) const { return b[i]; }
	Dn4 h2(int i) const { return c[i]; }
	Dn4 ha(int i) const { return d[i]; }
};
static bool rd(FILE *f, std::vector<float> &v) { return fread(v.data(), 4, v.size(), f) == v.size(); }
int main(int argc, char **argv)
{
	if(argc != 3) return 2;
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if(!in || !out) return 3;
	int32_t h[6]; float s[7];
	if(fread(h, 4, 6, in) != 6 || fread(s, 4, 7, in) != 7) return 4;
	const int width = h[0], height = h[1], radius = h[5];
	const bool have = h[3] != 0, rectify = h[4] != 0;
	const size_t n = (size_t)width * height;
	std::vector<float> C(n * 3), m2(n), cnt(n), A(n * 3), N(n * 3), P(n * 3), cam(35), hD(n * 3), hV(n), hn(n), hA(n * 3), hN(n * 3), hP(n * 3);
	std::vector<uint8_t> hit(n), hhit(n);
	if(!rd(in, C) || !rd(in, m2) || !rd(in, cnt) || !rd(in, A) || !rd(in, N) || !rd(in, P) || fread(hit.data(), 1, n, in) != n) return 4;
	if(!rd(in, cam) || !rd(in, hD) || !rd(in, hV) || !rd(in, hn) || !rd(in, hA) || !rd(in, hN) || !rd(in, hP) || fread(hhit.data(), 1, n, in) != n) return 4;
	const DenoiseParams prm{h[2], s[0], s[1]};
	if(!denoise_params_valid(prm) || !temporal_cap_valid(s[2])) return 5;
	if(rectify && !rectify_params_valid(radius, s[3])) return 6;
	const TemporalCamera tc = temporal_camera(&cam[0], &cam[3], &cam[19]);
	std::vector<Dn4> x0(n), x0b(n), x1(n), x2(n), xa(n), h0(n), h1(n), h2(n), ha(n);
	for(size_t i = 0; i < n; ++i)
	{
		x0[i] = denoise_prepare(C[3 * i], C[3 * i + 1], C[3 * i + 2], m2[i], cnt[i], A[3 * i], A[3 * i + 1], A[3 * i + 2]);
		x1[i] = Dn4{N[3 * i], N[3 * i + 1], N[3 * i + 2], hit[i] ? 1.0f : 0.0f};
		x2[i] = Dn4{P[3 * i], P[3 * i + 1], P[3 * i + 2], cnt[i]};
		xa[i] = Dn4{A[3 * i], A[3 * i + 1], A[3 * i + 2], 0.0f};
		h0[i] = Dn4{hD[3 * i], hD[3 * i + 1], hD[3 * i + 2], hV[i]};
		h1[i] = Dn4{hN[3 * i], hN[3 * i + 1], hN[3 * i + 2], hhit[i] ? 1.0f : 0.0f};
		h2[i] = Dn4{hP[3 * i], hP[3 * i + 1], hP[3 * i + 2], hn[i]};
		ha[i] = Dn4{hA[3 * i], hA[3 * i + 1], hA[3 * i + 2], 0.0f};
	}
	const Hist hist{h0.data(), h1.data(), h2.data(), ha.data()};
	const Img cur{x0.data(), x1.data(), x2.data(), xa.data()};
	std::vector<float> Dm(n * 3), Vm(n), no(n), kept(n), R0(n * 4), R1(n * 4);
	for(int y = 0; y < height; ++y)
		for(int x = 0; x < width; ++x)
		{
			const size_t i = (size_t)y * width + x;
			TemporalOut m;
			if(rectify)
			{
				const RectifyStats st = rectify_window(cur, width, height, x, y, radius, &s[4]);
				R0[4 * i] = st.r0.x; R0[4 * i + 1] = st.r0.y; R0[4 * i + 2] = st.r0.z; R0[4 * i + 3] = st.r0.w;
				R1[4 * i] = st.r1.x; R1[4 * i + 1] = st.r1.y; R1[4 * i + 2] = st.r1.z; R1[4 * i + 3] = st.r1.w;
				m = temporal_merge(hist, have, tc, width, height, x0[i], x1[i], x2[i], xa[i], x2[i].w, s[2], Rectify{true, st.r0, st.r1, s[3]});
			}
			else m = temporal_merge(hist, have, tc, width, height, x0[i], x1[i], x2[i], xa[i], x2[i].w, s[2]);
			x0b[i] = m.x0; no[i] = m.n; kept[i] = m.kept;
			Dm[3 * i] = m.x0.x; Dm[3 * i + 1] = m.x0.y; Dm[3 * i + 2] = m.x0.z; Vm[i] = m.x0.w;
		}
	x0.swap(x0b);
	for(int l = 0; l < prm.levels; ++l)
	{
		const Img img{x0.data(), x1.data(), x2.data(), xa.data()};
		for(int y = 0; y < height; ++y)
			for(int x = 0; x < width; ++x) x0b[(size_t)y * width + x] = denoise_level(img, width, height, x, y, 1 << l, prm.sigma_l, prm.sigma_z);
		x0.swap(x0b);
	}
	std::vector<float> rgb(n * 3);
	for(size_t i = 0; i < n; ++i) denoise_remodulate(x0[i], xa[i], &rgb[3 * i]);
	for(const std::vector<float> *v : {&Dm, &Vm, &no, &kept, &R0, &R1, &rgb}) fwrite(v->data(), 4, v->size(), out);
	fclose(out);
	return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("rectify_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", DEVICE, src, "-o", exe])
    return exe, str(d)


def run_driver(driver, call, hist, cam, rectify=True, radius=3, gamma=1.0, cap=64.0, levels=5, sigma_l=4.0, sigma_z=0.1):
    """One temporal call of the header, rectified or not: dict(D, V, n, kept, R0, R1, rgb)."""
    exe, d = driver
    C, m2, n, A, N, P, hit = call
    h, w = np.shape(m2)
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).tobytes()  # noqa: E731
    u8 = lambda a: np.ascontiguousarray(a).astype(np.uint8).tobytes()  # noqa: E731
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([w, h, levels, 0 if hist is None else 1, 1 if rectify else 0, radius], np.int32).tobytes())
        f.write(np.array([sigma_l, sigma_z, cap, gamma], np.float32).tobytes() + f32(cam[0]))
        f.write(b"".join(f32(a) for a in (C, m2, n, A, N, P)) + u8(hit))
        if hist is None:
            f.write(bytes(4 * 35 + (3 + 1 + 1 + 3 + 3 + 3) * 4 * h * w + h * w))
        else:
            f.write(f32(hist["raw_cam"]) + b"".join(f32(hist[k]) for k in ("D", "V", "n", "A", "N", "P")) + u8(hist["hit"]))
    subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    o = np.fromfile(os.path.join(d, "out.bin"), dtype=np.float32)
    k, out, at = h * w, {}, 0
    for name, c in (("D", 3), ("V", 1), ("n", 1), ("kept", 1), ("R0", 4), ("R1", 4), ("rgb", 3)):
        out[name] = o[at:at + c * k].reshape((h, w, c) if c > 1 else (h, w))
        at += c * k
    assert at == o.size
    return out


def check(driver, call, hist, cam, **kw):
    """The header and numpy on one rectified call: zero differing words in merged D, V, n_out, kept, R0, R1 and the result.  Returns numpy's
    (result, n_out, the history the call would commit, dict(kept, R0, R1, ...))."""
    got = run_driver(driver, call, hist, cam, **kw)
    want, want_n, new, extra = RT.denoise(*call, hist, cam, **kw)
    for name, exp in (("D", new["D"]), ("V", new["V"]), ("n", want_n), ("kept", extra["kept"]), ("R0", extra["R0"]), ("R1", extra["R1"]), ("rgb", want)):
        assert differing(got[name], exp) == 0, "%s: %d words differ from the numpy restatement (%s)" % (name, differing(got[name], exp), kw)
    new["raw_cam"] = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in cam])
    return want, want_n, new, extra


def test_header_needs_no_hip_include_and_has_no_fma_exp_or_pow(tmp_path):
    text = open(os.path.join(DEVICE, "rectify.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in "".join(l for l in code.splitlines() if l.startswith("#include")).lower()
    assert not re.search(r"\b(fmaf?|expf?|exp2f?|powf?|__builtin\w*)\b", code)
    assert re.search(r'#include "rectify.hpp"', open(os.path.join(DEVICE, "temporal.hpp")).read())
    program = (b'#include "temporal.hpp"\nusing namespace adypt;\n'
               b"static_assert(kRectifyMinTaps == 4 && kRectifyDefaultRadius == 3 && kRectifyDefaultGamma == 1.0f, \"the definition's constants\");\n"
               b"int main() { return rectify_params_valid(kRectifyDefaultRadius, kRectifyDefaultGamma) && !rectify_params_valid(0, 1.0f) && !rectify_params_valid(4, 1.0f)"
               b" && rectify_params_valid(1, 0.0f) && !rectify_params_valid(3, -1.0f) && !rectify_params_valid(3, 0.0f / 0.0f) && !rectify_params_valid(3, 1.0f / 0.0f) ? 0 : 1; }\n")
    exe = str(tmp_path / "rectify_params")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-Wno-div-by-zero", "-I", DEVICE, "-x", "c++", "-", "-o", exe], input=program, check=True)
    assert subprocess.run([exe]).returncode == 0, "rectify_params_valid"


# ---- sequences of cameras, everything made by the CPU oracle ----
SUNS = (1.0, 0.25, 4.0)
_poses = {}


def oracle_sequences(scene_cache, sobol_matrices, key, n_cameras=4, spp=4):
    """{sun scale: ([(call inputs, camera)] of the four cameras, the oracle's 1024-spp image of the last)}: the cameras, seeds and sample counts of
    tests/test_temporal_definition.py; the first three poses under the config's sun, the last under the sun times the scale.  Once per scene."""
    if key in _poses:
        return _poses[key]
    from adypt_amd import api, scenes
    name, w, h, life, axis = TD.SEQUENCES[key]
    spec = scenes.make_scene(name, scene_cache, width=w, height=h, pt={"tmpLifetime": life, "maxBounce": 6, "subpixel": 1})
    cfg = api.InstanceConfig()
    assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
    sc = api.Scene()
    assert sc.LoadFromFile(cfg.m_obj_filename)
    b = api.WideBVH()
    if not b.LoadFromFile(cfg.m_bvh_filename, cfg.bvh_params()):
        b.Build(sc, cfg.bvh_params())
        assert b.SaveToFile(cfg.m_bvh_filename, cfg.bvh_params())
    osc = O.Scene(b.nodes, b.tri_indices, sc.triangles, sc.materials, textures=sc.textures)
    c = cfg.c
    yaw0, pos0, sun0 = c.yaw, list(c.position), [F(v) for v in c.sun]
    assert max(sun0) > 0, "the scene has no sun to change"

    def pose(k, scale, converge):
        c.yaw = yaw0 + TD.STEP_YAW * k
        pos = list(pos0)
        pos[axis] += TD.STEP_MOVE * k
        for i in range(3):
            c.position[i] = pos[i]
            c.sun[i] = sun0[i] * F(scale)
        P, shift = T.oracle_params(c), O.shift_bytes(SEED + k, w, h)  # a seed of its own per camera
        samples = T.frame_samples(osc, P, shift, sobol_matrices, spp)
        _, m2 = T.moments(samples)
        state = O.PathTracerState(w, h)
        O.pt_frames(osc, P, shift, sobol_matrices, state, spp)
        guides = [O.primary_frame(osc, P, t) for t in (0, 4, 5)]
        hit = guides[0][1]["tri_id"] != -1
        call = (state.accum[..., :3].copy(), m2, spp, guides[0][0][..., :3].copy(), guides[1][0][..., :3].copy(), guides[2][0][..., :3].copy(), hit)
        ip, iv = O.camera(c.fov, c.yaw, c.pitch, w, h)
        ref = None
        if converge:
            O.pt_frames(osc, P, shift, sobol_matrices, state, 1024 - state.spp)
            ref = state.accum[..., :3].copy()
        return (call, (np.array(pos, np.float32), ip, iv)), ref

    first = [pose(k, 1.0, False)[0] for k in range(n_cameras - 1)]
    out = {}
    for scale in SUNS:
        last, ref = pose(n_cameras - 1, scale, True)
        out[scale] = (first + [last], ref)
    _poses[key] = out
    return out


@pytest.mark.parametrize("key", ["sibenik", "tiny0"])
def test_oracle_sequences_are_bit_exact_and_stale_light_is_rectified(key, driver, scene_cache, sobol_matrices):
    """Four cameras a step apart, 4 spp each, a seed per camera, committing, cap 64, 5 levels, radius 3, gamma 1, the flag given to all four calls; the
    last pose under the config's sun, a quarter of it and four times it.  Header against numpy: zero differing words at every step.  Against the
    oracle's 1024-spp image of the last pose: under a quarter of the sun the rectified error is strictly below the plain temporal call's on both scenes
    and on tiny0 at most half of it; under the unchanged sun on sibenik it is strictly below the spatial filter's alone.
    Measured, printed by this test and quoted in DESIGN.md section 4, Rectifying stale history (rmse raw / spatial only / temporal / rectified):
        sibenik 96x54   sun x 1     0.5305 / 0.1655 / 0.1111 / 0.1320
                        sun x 0.25  0.3773 / 0.1221 / 0.1628 / 0.1073
                        sun x 4     0.6828 / 0.2118 / 0.1623 / 0.1637
        tiny0 100x75    sun x 1     0.5699 / 0.2209 / 0.2011 / 0.2000
                        sun x 0.25  0.2905 / 0.1045 / 0.6551 / 0.1210
                        sun x 4     0.6914 / 0.2717 / 0.6495 / 0.3027"""
    sequences = oracle_sequences(scene_cache, sobol_matrices, key)
    err = {}
    for scale in SUNS:
        calls, ref = sequences[scale]
        hist = plain_hist = None
        for call, cam in calls:
            out, n_out, hist, extra = check(driver, call, hist, cam)
            plain, plain_n, plain_hist = TT.denoise(*call, plain_hist, cam)
        assert np.isfinite(out).all() and np.isfinite(extra["kept"]).all()
        hit = call[6]
        assert (extra["kept"][~hit] == F(1)).all() and (extra["kept"] >= 0).all() and (extra["kept"] <= F(1)).all() and (n_out <= plain_n).all()
        err[scale] = raw, spatial, temporal, rectified = D.rmse(call[0], ref), D.rmse(D.denoise(*call), ref), D.rmse(plain, ref), D.rmse(out, ref)
        print("%s, last pose sun x %g: rmse raw %.4f spatial only %.4f temporal %.4f rectified %.4f (rectified / temporal %.3f, / spatial %.3f), kept < 1 on %.1f %% of the hit pixels"
              % (key, scale, raw, spatial, temporal, rectified, rectified / temporal, rectified / spatial, 100.0 * float((extra["kept"][hit] < 1).mean())))
    assert err[0.25][3] < err[0.25][2]
    if key == "tiny0":
        assert err[0.25][3] <= 0.5 * err[0.25][2]
    if key == "sibenik":
        assert err[1.0][3] < err[1.0][1]


# ---- hand-made cases ----
wall, camera_of = TD.wall, TD.camera_of


def history_of(driver, call, cam, **kw):
    return check(driver, call, None, cam, **kw)[2]


def same_as_plain(call, hist, cam, out, n_out, new, where, **kw):
    """wherever `where`, the merged words and n_out are the plain temporal call's"""
    _, plain_n, plain = TT.denoise(*call, hist, cam, **kw)
    for name, a, b in (("D", new["D"], plain["D"]), ("V", new["V"], plain["V"]), ("n_out", n_out, plain_n)):
        assert differing(a[where], b[where]) == 0, name


def window_size(h, w, radius):
    """the number of pixels of every pixel's window that lie inside the image"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((np.minimum(xx + radius, w - 1) - np.maximum(xx - radius, 0) + 1) * (np.minimum(yy + radius, h - 1) - np.maximum(yy - radius, 0) + 1)).astype(np.float32)


def test_hand_made_cases(driver):
    rs = np.random.RandomState(12)
    # 1 x 1: one tap, fewer than kRectifyMinTaps — the plain temporal call's bits; 2 x 3: six taps, only just enough at every radius
    for (h, w), enough in (((1, 1), False), ((2, 3), True)):
        cam = camera_of(w=w, h=h)
        hist = history_of(driver, wall(rs, h, w, cam), cam)
        call = wall(rs, h, w, cam)
        for radius in (1, 2, 3):
            out, n_out, new, extra = check(driver, call, hist, cam, radius=radius)
            assert np.isfinite(out).all() and np.array_equal(extra["R0"][..., 3], window_size(h, w, radius)) and (extra["R0"][..., 3] >= F(4)).all() == enough
            if not enough:
                plain, plain_n, plain_new = TT.denoise(*call, hist, cam)
                assert differing(out, plain) == 0 and differing(n_out, plain_n) == 0 and differing(new["D"], plain_new["D"]) == 0 and (extra["kept"] == F(1)).all()
            same_as_plain(call, hist, cam, out, n_out, new, extra["kept"] == F(1))
    h, w = 9, 13
    cam = camera_of()
    hist = history_of(driver, wall(rs, h, w, cam), cam)
    # a window crossing every image border: the tap counts are the clipped windows' sizes at every radius
    call = wall(rs, h, w, cam)
    for radius in (1, 2, 3):
        out, n_out, new, extra = check(driver, call, hist, cam, radius=radius)
        assert np.array_equal(extra["R0"][..., 3], window_size(h, w, radius)) and np.isfinite(out).all()
        same_as_plain(call, hist, cam, out, n_out, new, extra["kept"] == F(1))
    assert (extra["kept"] < F(1)).any() and (extra["kept"] == F(1)).any()  # (random radiance under 8 spp: both kinds of pixel)
    # nothing but sky: k = 0 everywhere, nothing is rectified
    sky = wall(rs, h, w, cam)
    sky[6][:] = False
    for k in (3, 4, 5):
        sky[k][:] = 0
    out, n_out, _, extra = check(driver, sky, history_of(driver, sky, cam), cam)
    assert (extra["R0"] == 0).all() and (extra["R1"] == 0).all() and (extra["kept"] == F(1)).all() and (n_out == F(8)).all()
    # a flat wall (var = 0, no sampling noise: the limit is 0) and a history that differs: the history is dropped, n_out == n, the merged words the call's own
    floor = F(0.5) + F(0.01)  # (what prepare divides the radiance by: D0 = 2 and 0.5, whose sums and squares are exact)
    flat = wall(rs, h, w, cam)
    flat[0][:] = floor * F(2.0)
    flat[1][:] = 0
    other = wall(rs, h, w, cam)
    other[0][:] = floor * F(0.5)
    other[1][:] = 0
    out, n_out, new, extra = check(driver, flat, history_of(driver, other, cam), cam)
    assert (extra["R1"] == 0).all() and (extra["kept"] == 0).all() and (n_out == F(8)).all()
    assert differing(out, D.denoise(*flat)) == 0, "a dropped history left a trace"
    # ... and a history that agrees to the bit is kept whole
    out, n_out, new, extra = check(driver, flat, history_of(driver, flat, cam), cam)
    assert (extra["kept"] == F(1)).all() and (n_out == F(16)).all()
    # gamma = 0: every history that is not the window's mean to the bit is dropped
    call = wall(rs, h, w, cam)
    out, n_out, new, extra = check(driver, call, hist, cam, gamma=0.0)
    assert (extra["kept"] == 0).all() and (n_out == F(8)).all() and differing(out, D.denoise(*call)) == 0
    # a large gamma keeps everything: the plain temporal call
    out, n_out, new, extra = check(driver, call, hist, cam, gamma=1.0e6)
    assert (extra["kept"] == F(1)).all()
    same_as_plain(call, hist, cam, out, n_out, new, np.ones((h, w), bool))
    # NaN in P, in N, in the current D0 (through C) and V0 (through m2), and in the history: it spreads nowhere, everything else stays finite
    call = wall(rs, h, w, cam)
    call[5][2, 3, 1] = np.nan
    call[4][6, 7, 0] = np.nan
    call[0][4, 4, 2] = np.nan
    call[0][4, 10, 0] = np.inf
    call[1][7, 5] = np.nan
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in hist.items()}
    for i, k in enumerate(("D", "V", "n", "P", "N", "A")):
        bad[k][1 + i, 9] = np.nan
    got = run_driver(driver, call, bad, cam)
    want, want_n, new, extra = RT.denoise(*call, bad, cam)
    for name, exp in (("D", new["D"]), ("V", new["V"]), ("n", want_n), ("kept", extra["kept"]), ("R0", extra["R0"]), ("R1", extra["R1"])):
        assert differing(got[name], exp) == 0, name
    # (the a-trous levels carry a pixel's own NaN radiance on to its neighbours, as they always did: the result is compared as numbers)
    assert np.array_equal(np.isnan(got["rgb"]), np.isnan(want)) and differing(np.nan_to_num(got["rgb"]), np.nan_to_num(want)) == 0
    own = np.zeros((h, w), bool)  # the pixels whose own values are not numbers
    for y, x in ((4, 4), (4, 10), (7, 5)):
        own[y, x] = True
    assert np.isfinite(extra["R0"]).all() and np.isfinite(extra["R1"]).all() and np.isfinite(extra["kept"]).all() and np.isfinite(want_n).all()
    assert np.isfinite(new["D"][~own]).all() and np.isfinite(new["V"][~own]).all()
    assert extra["R0"][2, 3, 3] == 0 and extra["R0"][6, 7, 3] == 0 and want_n[2, 3] == F(8) and want_n[6, 7] == F(8)  # (a NaN surface counts no tap, its own included)
    clean = wall(rs, h, w, cam)
    assert RT.denoise(*clean, bad, cam)[3]["R0"][4, 4, 3] == F(49) and extra["R0"][4, 4, 3] == F(45)  # (left out: its own NaN radiance, the NaN point, the NaN normal, the NaN variance)
    # an emitter column (albedo 0, demodulated by the floor: radiance 5000) next to a wall: the albedo test keeps it out of the wall's statistics
    scene = wall(rs, h, w, cam)
    scene[3][:, 6] = 0
    scene[0][:, 6] = 50.0
    out, n_out, new, extra = check(driver, scene, history_of(driver, scene, cam), cam)
    wall_px = np.ones((h, w), bool)
    wall_px[:, 6] = False
    assert extra["R0"][wall_px][:, :3].max() < 4.1 and extra["R0"][:, 6, :3].min() > 4000.0  # (the wall: radiance below 2 over albedo 0.51)
    assert np.array_equal(extra["R0"][:, 6, 3], window_size(h, 1, 3)[:, 0])  # the column's own taps only
    assert np.isfinite(out).all() and out[wall_px].max() < 10.0


def test_the_new_symbols_are_declared_and_bound():
    from adypt_amd import _native as N
    header = open(os.path.join(ROOT, "include", "adypt_hip.h")).read()
    for stem in ("denoise_temporal_rectified", "read_denoise_rectify", "get_denoise_rectify"):
        for name in ("adypt_" + stem, "adypt_multi_" + stem):
            assert re.search(r"\bint %s\(" % name, header), name
            assert name in N.EXPORTS and hasattr(N.lib, name), name
    assert "typedef struct adypt_rectify_params" in header and "typedef struct adypt_denoise_rectify" in header and N.lib.adypt_abi_version() == 4
    assert ctypes.sizeof(N.RectifyParams) == 8 and ctypes.sizeof(N.DenoiseRectify) == 24
    assert ctypes.sizeof(N.TemporalParams) == 8 and ctypes.sizeof(N.DenoiseParams) == 12 and ctypes.sizeof(N.DenoiseMotion) == 24
    from adypt_amd import api
    import inspect
    sig = inspect.signature(api.HipPathTracer.Denoise)
    assert [sig.parameters[k].default for k in ("rectify", "rectify_radius", "rectify_gamma")] == [False, 3, 1.0]
    assert hasattr(api.HipPathTracer, "ReadDenoiseRectify") and hasattr(api.HipPathTracer, "GetDenoiseRectify")


def test_the_named_edge_inputs(driver):
    """tests/denoise_edge_inputs.py's entries for the window statistics and the rectified merge — every radius at the sizes round the 32 x 8 workgroup, a tap
    refused by each test of rectify_tap in turn, sums that overflow, a limit that is no number, one clamped channel, kept = 0 — each reaching its branch
    by the truth's account: zero differing words."""
    from tests import denoise_edge_inputs as E  # (here: the module imports this file's generators)
    for name, case in E.rectify_cases().items():
        assert case["reach"](E.rectify_truth(case)), name + ": the case does not reach what it is named after"
        for radius in ((1, 2, 3) if name.startswith("size-") else (case["kw"].get("radius", 3),)):
            kw = dict(case["kw"], radius=radius)
            try:
                if np.isfinite(case["call"][0]).all() and np.isfinite(case["call"][1]).all():
                    check(driver, case["call"], case["hist"], case["cam"], **kw)
                else:
                    # radiance or moments that are no numbers: the window and the merge are held word for word; the levels carry the pixel's own NaN on to
                    # its neighbours, and the result is compared as numbers (as test_hand_made_cases does)
                    got = run_driver(driver, case["call"], case["hist"], case["cam"], **kw)
                    want, want_n, new, extra = RT.denoise(*case["call"], case["hist"], case["cam"], **kw)
                    own = ~np.isfinite(new["D"]).all(-1) | ~np.isfinite(new["V"])  # the pixels whose own values are no numbers
                    assert own.any() and not own.all()
                    for field, exp in (("D", new["D"]), ("V", new["V"]), ("n", want_n), ("kept", extra["kept"]), ("R0", extra["R0"]), ("R1", extra["R1"])):
                        keep = ~own if field in ("D", "V") else np.ones_like(own)
                        assert differing(got[field][keep], exp[keep]) == 0, field
                        assert np.array_equal(np.isnan(got[field]), np.isnan(exp)), field
                    assert np.array_equal(np.isnan(got["rgb"]), np.isnan(want)) and differing(np.nan_to_num(got["rgb"]), np.nan_to_num(want)) == 0, "rgb"
            except AssertionError as e:
                raise AssertionError("%s, radius %d: %s" % (name, radius, e))
