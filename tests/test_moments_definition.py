"""Variance from temporal moments: the definition (csrc/device/moments.hpp, and the moments form of the merge in csrc/device/temporal.hpp) compiled on
the host and held bit for bit against its numpy float32 restatement (tests/moments_truth.py): on sequences of cameras at 1 spp per pose whose images,
moments and guides the CPU oracle makes, and on hand-made edge cases.  Its quality is measured against the oracle's converged image at the last camera,
never against the code under test.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import denoise_truth as D
from tests import moments_truth as MT
from tests import noise_truth as T
from tests import temporal_motion_truth as TM
from tests import temporal_truth as TT
from tests import test_temporal_definition as TD  # (its camera steps, its hand-made walls)
from tests.helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
SEED = 31
F = np.float32

DRIVER = r"""
#include "temporal.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace adypt;
// IN:  int32 w, h, levels, have, motion; float32 sigma_l, sigma_z, cap, origin[3] (the current camera's);
//      the call:    float32 C[h][w][3], m2[h][w], n[h][w], A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
//      the history: float32 origin[3], inv_proj[16], inv_view[16], D[h][w][3], S[h][w], n[h][w], A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
//      motion != 0: float32 Pp[h][w][3], Np[h][w][3]; uint8 valid[h][w]   (temporal_previous_point's answer, made by the caller)
// OUT: float32 Dm[h][w][3], S[h][w], V[h][w], n_out[h][w], spatial[h][w] (0 / 1), rgb[h][w][3]
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
	int32_t h[5]; float s[6];
	if(fread(h, 4, 5, in) != 5 || fread(s, 4, 6, in) != 6) return 4;
	const int width = h[0], height = h[1];
	const bool have = h[3] != 0, motion = h[4] != 0;
	const size_t n = (size_t)width * height;
	std::vector<float> C(n * 3), m2(n), cnt(n), A(n * 3), N(n * 3), P(n * 3), cam(35), hD(n * 3), hS(n), hn(n), hA(n * 3), hN(n * 3), hP(n * 3), Pp(n * 3), Np(n * 3);
	std::vector<uint8_t> hit(n), hhit(n), valid(n);
	if(!rd(in, C) || !rd(in, m2) || !rd(in, cnt) || !rd(in, A) || !rd(in, N) || !rd(in, P) || fread(hit.data(), 1, n, in) != n) return 4;
	if(!rd(in, cam) || !rd(in, hD) || !rd(in, hS) || !rd(in, hn) || !rd(in, hA) || !rd(in, hN) || !rd(in, hP) || fread(hhit.data(), 1, n, in) != n) return 4;
	if(motion && (!rd(in, Pp) || !rd(in, Np) || fread(valid.data(), 1, n, in) != n)) return 4;
	const DenoiseParams prm{h[2], s[0], s[1]};
	if(!denoise_params_valid(prm) || !temporal_cap_valid(s[2])) return 5;
	const TemporalCamera tc = temporal_camera(&cam[0], &cam[3], &cam[19]);
	std::vector<Dn4> x0(n), xm(n), x0b(n), x1(n), x2(n), xa(n), h0(n), h1(n), h2(n), ha(n);
	for(size_t i = 0; i < n; ++i)
	{
		x0[i] = moments_prepare(C[3 * i], C[3 * i + 1], C[3 * i + 2], m2[i], cnt[i], A[3 * i], A[3 * i + 1], A[3 * i + 2]);
		x1[i] = Dn4{N[3 * i], N[3 * i + 1], N[3 * i + 2], hit[i] ? 1.0f : 0.0f};
		x2[i] = Dn4{P[3 * i], P[3 * i + 1], P[3 * i + 2], cnt[i]};
		xa[i] = Dn4{A[3 * i], A[3 * i + 1], A[3 * i + 2], 0.0f};
		h0[i] = Dn4{hD[3 * i], hD[3 * i + 1], hD[3 * i + 2], hS[i]};
		h1[i] = Dn4{hN[3 * i], hN[3 * i + 1], hN[3 * i + 2], hhit[i] ? 1.0f : 0.0f};
		h2[i] = Dn4{hP[3 * i], hP[3 * i + 1], hP[3 * i + 2], hn[i]};
		ha[i] = Dn4{hA[3 * i], hA[3 * i + 1], hA[3 * i + 2], 0.0f};
	}
	const Hist hist{h0.data(), h1.data(), h2.data(), ha.data()};
	std::vector<float> Dm(n * 3), Sm(n), V(n), no(n), sp(n);
	for(size_t i = 0; i < n; ++i)
	{
		const TemporalOut m = motion ? temporal_merge_motion<true>(hist, have, tc, width, height, x0[i], x1[i], xa[i], x2[i].w, s[2], Dn4{Pp[3 * i], Pp[3 * i + 1], Pp[3 * i + 2], 0.0f},
		                                                           Dn4{Np[3 * i], Np[3 * i + 1], Np[3 * i + 2], valid[i] ? 1.0f : 0.0f})
		                             : temporal_merge<true>(hist, have, tc, width, height, x0[i], x1[i], x2[i], xa[i], x2[i].w, s[2]);
		xm[i] = m.x0; no[i] = m.n;
		Dm[3 * i] = m.x0.x; Dm[3 * i + 1] = m.x0.y; Dm[3 * i + 2] = m.x0.z; Sm[i] = m.x0.w;
	}
	for(size_t i = 0; i < n; ++i) x2[i].w = no[i]; // (as k_temporal_merge leaves X2)
	{
		const Img img{xm.data(), x1.data(), x2.data(), xa.data()};
		for(int y = 0; y < height; ++y)
			for(int x = 0; x < width; ++x)
			{
				const size_t i = (size_t)y * width + x;
				const MomentsVariance r = moments_variance(img, width, height, x, y, &s[3]);
				V[i] = r.v; sp[i] = r.spatial ? 1.0f : 0.0f;
				x0[i] = Dn4{xm[i].x, xm[i].y, xm[i].z, r.v};
			}
	}
	for(int l = 0; l < prm.levels; ++l)
	{
		const Img img{x0.data(), x1.data(), x2.data(), xa.data()};
		for(int y = 0; y < height; ++y)
			for(int x = 0; x < width; ++x) x0b[(size_t)y * width + x] = denoise_level(img, width, height, x, y, 1 << l, prm.sigma_l, prm.sigma_z);
		x0.swap(x0b);
	}
	std::vector<float> rgb(n * 3);
	for(size_t i = 0; i < n; ++i) denoise_remodulate(x0[i], xa[i], &rgb[3 * i]);
	fwrite(Dm.data(), 4, Dm.size(), out); fwrite(Sm.data(), 4, Sm.size(), out); fwrite(V.data(), 4, V.size(), out); fwrite(no.data(), 4, no.size(), out);
	fwrite(sp.data(), 4, sp.size(), out); fwrite(rgb.data(), 4, rgb.size(), out);
	fclose(out);
	return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("moments_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", DEVICE, src, "-o", exe])
    return exe, str(d)


def run_driver(driver, call, hist, cam, through=None, cap=64.0, levels=5, sigma_l=4.0, sigma_z=0.1):
    """One moments call of the header: dict(D, S, V, n, spatial, rgb).  call = (C, m2, n, A, N, P, hit); hist: what the call FINDS (None: nothing);
    through: None, or (N_prev, P_prev, valid)."""
    exe, d = driver
    C, m2, n, A, N, P, hit = call
    h, w = np.shape(m2)
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).tobytes()  # noqa: E731
    u8 = lambda a: np.ascontiguousarray(a).astype(np.uint8).tobytes()  # noqa: E731
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([w, h, levels, 0 if hist is None else 1, 0 if through is None else 1], np.int32).tobytes())
        f.write(np.array([sigma_l, sigma_z, cap], np.float32).tobytes() + f32(np.asarray(cam[0]).reshape(3)))
        f.write(b"".join(f32(a) for a in (C, m2, n, A, N, P)) + u8(hit))
        if hist is None:
            f.write(bytes(4 * 35 + (3 + 1 + 1 + 3 + 3 + 3) * 4 * h * w + h * w))
        else:
            f.write(f32(hist["raw_cam"]) + b"".join(f32(hist[k]) for k in ("D", "V", "n", "A", "N", "P")) + u8(hist["hit"]))
        if through is not None:
            f.write(f32(through[1]) + f32(through[0]) + u8(through[2]))
    subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    o = np.fromfile(os.path.join(d, "out.bin"), dtype=np.float32)
    k = h * w
    return dict(D=o[:3 * k].reshape(h, w, 3), S=o[3 * k:4 * k].reshape(h, w), V=o[4 * k:5 * k].reshape(h, w), n=o[5 * k:6 * k].reshape(h, w),
                spatial=o[6 * k:7 * k].reshape(h, w) != 0, rgb=o[7 * k:].reshape(h, w, 3))


def differing(a, b):
    return int((bits(np.ascontiguousarray(a, np.float32)) != bits(np.ascontiguousarray(b, np.float32))).sum())


def check(driver, call, hist, cam, motion=None, **kw):
    """The header and numpy on one moments call: zero differing words in the merged D and S, the variance, n_out and the result, and the same pixels
    spatial.  hist: what the last committing call of any kind left.  Returns numpy's (result, n_out, history the call would commit, extra)."""
    found = MT.history_for(hist, True)
    through = None
    if motion is not None:
        tri, uv, cur = motion
        Pp, _, Np, valid = TM.previous_point(None if found is None else found.get("tris"), cur, tri, uv, np.asarray(call[4], np.float32), np.asarray(call[5], np.float32))
        through = (Np, Pp, valid)
    got = run_driver(driver, call, found, cam, through, **kw)
    want, want_n, new, extra = MT.denoise(*call, hist, cam, motion=motion, **kw)
    for name, a, b in (("merged D", got["D"], extra["D"]), ("merged S", got["S"], extra["S"]), ("variance", got["V"], extra["V"]), ("history length", got["n"], want_n),
                       ("result", got["rgb"], want)):
        assert differing(a, b) == 0, "%s: %d words differ from the numpy restatement (%s)" % (name, differing(a, b), kw)
    assert np.array_equal(got["spatial"], extra["spatial"]), "other pixels took the window estimate than numpy says"
    new["raw_cam"] = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in cam])
    return want, want_n, new, extra


def test_header_needs_no_hip_include_and_has_no_fma_exp_or_pow():
    text = open(os.path.join(DEVICE, "moments.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in "".join(l for l in code.splitlines() if l.startswith("#include")).lower()
    assert not re.search(r"\b(fmaf?|expf?|exp2f?|powf?|__builtin\w*)\b", code)
    for name, value in (("kMomentsMinLength", 4), ("kMomentsRadius", 3), ("kMomentsMinTaps", 4)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), code), name
    assert '#include "moments.hpp"' in open(os.path.join(DEVICE, "temporal.hpp")).read()
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", DEVICE, "-x", "c++", "-"],
                   input=b'#include "temporal.hpp"\nint main() { return adypt::moments_wants_window(true, 3.99f) && !adypt::moments_wants_window(true, 4.0f) ? 0 : 1; }\n', check=True)


# ---- sequences of cameras, everything made by the CPU oracle ----
N_CAMERAS, MAX_SPP = 12, 3
_sequence = {}


def oracle_sequence(scene_cache, sobol_matrices, key):
    """{spp: call inputs} and (origin, inv_proj, inv_view) of N_CAMERAS cameras a step of tests/test_temporal_definition.py apart, each with the seed
    SEED + k, after 1 .. MAX_SPP frames; and the oracle's 1024-spp image at the last.  Once per scene."""
    if key in _sequence:
        return _sequence[key]
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
    yaw0, pos0 = c.yaw, list(c.position)
    poses, ref = [], None
    for k in range(N_CAMERAS):
        c.yaw = yaw0 + TD.STEP_YAW * k
        pos = list(pos0)
        pos[axis] += TD.STEP_MOVE * k
        for i in range(3):
            c.position[i] = pos[i]
        P, shift = T.oracle_params(c), O.shift_bytes(SEED + k, w, h)
        samples = T.frame_samples(osc, P, shift, sobol_matrices, MAX_SPP)
        guides = [O.primary_frame(osc, P, t) for t in (0, 4, 5)]
        hit = guides[0][1]["tri_id"] != -1
        state, calls = O.PathTracerState(w, h), {}
        for spp in range(1, MAX_SPP + 1):
            O.pt_frames(osc, P, shift, sobol_matrices, state, 1)
            _, m2 = T.moments(samples[:spp])
            calls[spp] = (state.accum[..., :3].copy(), m2, spp, guides[0][0][..., :3].copy(), guides[1][0][..., :3].copy(), guides[2][0][..., :3].copy(), hit)
        ip, iv = O.camera(c.fov, c.yaw, c.pitch, w, h)
        poses.append((calls, (np.array(pos, np.float32), ip, iv)))
        if k == N_CAMERAS - 1:
            O.pt_frames(osc, P, shift, sobol_matrices, state, 1024 - state.spp)
            ref = state.accum[..., :3].copy()
    _sequence[key] = (poses, ref)
    return _sequence[key]


@pytest.mark.parametrize("key", ["sibenik", "tiny0"])
def test_oracle_sequences_are_bit_exact(key, driver, scene_cache, sobol_matrices):
    """Twelve cameras a step apart at 1 spp each, a seed per camera, committing: the header agrees with numpy in every word of the merged D and S, of V,
    of n_out and of the result at every step; and once more with 1 and 3 spp alternating.  At the first pose every hit pixel asks its window; at the
    last, under cap 64, only what found little or no history does."""
    poses, _ = oracle_sequence(scene_cache, sobol_matrices, key)
    for spps in ([1] * N_CAMERAS, [1, 3] * (N_CAMERAS // 2)):
        hist, shares = None, []
        for (calls, cam), spp in zip(poses, spps):
            out, n_out, hist, extra = check(driver, calls[spp], hist, cam)
            assert np.isfinite(out).all() and np.isfinite(extra["V"]).all() and (extra["V"] >= 0).all()
            hit = calls[spp][6]
            shares.append(float(extra["spatial"][hit].mean()))
        print("%s, spp %s: share of the hit pixels that took the window estimate, per pose: %s" % (key, spps[:2], " ".join("%.3f" % s for s in shares)))
        if spps[0] == 1:
            assert shares[0] > 0.9 and shares[-1] < 0.2 and shares[-1] < shares[0]


def test_a_sequence_through_follow_motion_is_bit_exact(driver):
    """tests/test_temporal_motion_definition.py's hand-made scene at 1 spp: a committing moments call before the triangles move, then the call after,
    merged through the previous point temporal_motion_truth gives: the moved region keeps its history."""
    from tests import test_temporal_motion_definition as TMD
    before, cam, after, tri, uv, prev, cur, region = TMD.scene()
    before, after = list(before), list(after)
    before[2], after[2] = 1, 1
    _, n0, hist, _ = check(driver, before, None, cam, motion=(tri, uv, prev))
    assert (n0 == F(1)).all() and hist["moments"] and "tris" in hist
    _, n_follow, _, extra = check(driver, after, hist, cam, motion=(tri, uv, cur))
    _, n_plain, _, _ = check(driver, after, hist, cam)
    moved = (TM.previous_point(prev, cur, tri, uv, np.asarray(after[4], np.float32), np.asarray(after[5], np.float32))[1])
    assert moved.any() and (n_follow[moved] > F(1)).mean() > (n_plain[moved] > F(1)).mean(), "following the motion found no more history on what moved"
    assert differing(n_follow[~moved], n_plain[~moved]) == 0


def rmse_of(poses, ref, spp, moments, history=True, window=True):
    """rmse against `ref` of the last pose's result after the whole sequence at `spp` per pose (history=False: the last pose alone)."""
    hist = None
    for calls, cam in (poses if history else poses[-1:]):
        if moments:
            out, _, hist, _ = MT.denoise(*calls[spp], hist, cam, window=window)
        else:
            out, _, hist = TT.denoise(*calls[spp], hist, cam)
    return D.rmse(out, ref)


# the thresholds: the bit-exact restatement's own ratios (below) plus 10 %, which covers only a later change of the oracle scenes' generators
LIMITS = {"sibenik": dict(history=0.510 * 1.1, to_2spp=1.075 * 1.1), "tiny0": dict(history=0.793 * 1.1, to_2spp=1.150 * 1.1)}


@pytest.mark.parametrize("key", ["sibenik", "tiny0"])
def test_quality_against_the_converged_image(key, scene_cache, sobol_matrices):
    """rmse against the oracle's 1024 spp at the last of the twelve cameras, cap 64, the default filter.  Measured, printed by this test and quoted in
    DESIGN.md section 4, Variance from temporal moments (raw 1 spp / moments call without history / with 12 poses of history / the same without the
    spatial window / the existing temporal call at 2 spp per pose; with / without history; 1-spp moments / 2-spp temporal):
        sibenik 96x54   1.0636 / 0.3027 / 0.1543 / 0.2272 / 0.1436   0.510   1.075
        tiny0 100x75    1.1702 / 0.3925 / 0.3114 / 0.3125 / 0.2707   0.793   1.150"""
    poses, ref = oracle_sequence(scene_cache, sobol_matrices, key)
    raw = D.rmse(poses[-1][0][1][0], ref)
    none, with_history = rmse_of(poses, ref, 1, True, history=False), rmse_of(poses, ref, 1, True)
    no_window, at_2spp = rmse_of(poses, ref, 1, True, window=False), rmse_of(poses, ref, 2, False)
    print("%s: rmse raw %.4f no history %.4f with history %.4f without the window %.4f temporal at 2 spp %.4f; with / without history %.3f, to 2 spp %.3f"
          % (key, raw, none, with_history, no_window, at_2spp, with_history / none, with_history / at_2spp))
    assert with_history < none < raw
    if key == "sibenik":
        assert with_history < no_window
    assert with_history / none <= LIMITS[key]["history"]
    assert with_history / at_2spp <= LIMITS[key]["to_2spp"]


# ---- hand-made cases ----
def history_of(driver, call, cam, **kw):
    return check(driver, call, None, cam, **kw)[2]


def wall(rs, h, w, cam, n=1, **kw):
    return TD.wall(rs, h, w, cam, n=n, **kw)


def test_hand_made_cases(driver):
    rs = np.random.RandomState(17)
    # the smallest images (the 7 x 7 window clipped on all four sides), the camera unchanged: a first call and one on its history
    for h, w in ((1, 1), (2, 3), (4, 4)):
        cam = TD.camera_of(w=w, h=h)
        _, _, hist, first = check(driver, wall(rs, h, w, cam), None, cam)
        assert first["spatial"].all() == (h * w >= 4) and (first["k"] == F(h * w)).all(), "every pixel of the wall counts, and no tap outside the image"
        out, n_out, _, extra = check(driver, wall(rs, h, w, cam), hist, cam)
        assert np.isfinite(out).all() and (n_out > F(1)).all()
    h, w = 9, 13
    cam = TD.camera_of()
    # nothing but sky, now and before: own / n, no window, no history
    sky = wall(rs, h, w, cam)
    sky[6][:] = False
    for k in (3, 4, 5):
        sky[k][:] = 0
    hist = history_of(driver, sky, cam)
    out, n_out, _, extra = check(driver, sky, hist, cam)
    assert np.isfinite(out).all() and (n_out == F(1)).all() and not extra["spatial"].any() and (extra["k"] == F(0)).all()
    # a miss centre among hits; windows of 3 and of 4 counting taps (an L of three hit pixels and a square of four, the rest sky)
    few = wall(rs, h, w, cam, n=2)
    few[6][:] = False
    for y, x in ((1, 1), (1, 2), (2, 1), (6, 8), (6, 9), (7, 8), (7, 9)):
        few[6][y, x] = True
    _, _, _, extra = check(driver, few, None, cam)
    assert (extra["k"][1, 1], extra["k"][1, 2], extra["k"][2, 1]) == (F(3),) * 3 and not extra["spatial"][:3, :3].any(), "a window of 3 taps decided"
    assert (extra["k"][6:8, 8:10] == F(4)).all() and extra["spatial"][6:8, 8:10].all() and int(extra["spatial"].sum()) == 4, "a window of 4 taps did not"
    own = np.maximum(extra["S"] - D.lum(extra["D"]) ** 2, 0)
    assert differing(extra["V"][~extra["spatial"]], (own / F(2))[~extra["spatial"]]) == 0 and (extra["V"][~few[6]] > 0).any()
    # n_out on both sides of kMomentsMinLength: histories of length 2.99 and 3 under an unchanged camera
    base = history_of(driver, wall(rs, h, w, cam), cam)
    short = dict(base, n=np.where(np.arange(w)[None, :] < 6, F(2.99), F(3.0)).astype(np.float32) * np.ones((h, w), np.float32))
    _, n_out, _, extra = check(driver, wall(rs, h, w, cam), short, cam)
    left, right = n_out[:, :5], n_out[:, 7:]
    assert (left > F(3.9)).all() and (left < F(4)).all() and extra["spatial"][:, :5].all(), "3.99: the window"
    assert (right == F(4)).any() and not extra["spatial"][:, 7:][right >= F(4)].any() and extra["spatial"][:, 7:][right < F(4)].all(), "4: the moments"
    # history_cap 2: no pixel ever leaves the window
    hist = None
    for _ in range(4):
        _, n_out, hist, extra = check(driver, wall(rs, h, w, cam), hist, cam, cap=2.0)
        assert (n_out <= F(3)).all() and extra["spatial"].all()
    # S < lum(D)^2: a long history whose S is 0 — own is floored at 0, and so is V
    low = dict(base, n=np.full((h, w), 10, np.float32), V=np.zeros((h, w), np.float32))
    _, n_out, _, extra = check(driver, wall(rs, h, w, cam), low, cam)
    below = (extra["S"] - D.lum(extra["D"]) ** 2) < 0
    assert (n_out > F(10.9)).all() and below.sum() > h * w // 2 and (extra["V"][below] == F(0)).all() and (extra["V"] >= F(0)).all() and not extra["spatial"].any()
    # a NaN or an infinity in the history's S, D or n of one pixel each: that tap is refused, nothing spreads
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    bad["V"][1, 9], bad["D"][2, 9, 1], bad["n"][3, 9] = np.nan, np.nan, np.nan
    bad["V"][5, 3], bad["D"][6, 3, 0], bad["n"][7, 3] = np.inf, -np.inf, np.inf
    out, n_out, new, extra = check(driver, wall(rs, h, w, cam), bad, cam)
    for a in (out, n_out, extra["D"], extra["S"], extra["V"]):
        assert np.isfinite(a).all()
    assert (n_out[[1, 2, 3, 5, 6, 7], [9, 9, 9, 3, 3, 3]] == F(1)).all() and (n_out > F(1)).sum() >= h * w - 6 * 4
    # a NaN in the CALL's colour stays in its own pixel's S and is refused as a tap of every window, its own included
    call = wall(rs, h, w, cam)
    call[0][4, 6, 1] = np.nan
    _, _, _, extra = check(driver, call, None, cam)
    assert np.isnan(extra["S"][4, 6]) and np.isfinite(extra["V"]).all(), "the pixel's own window goes without it too"
    assert extra["k"][4, 6] == F(48) and extra["k"][4, 5] == F(48) and extra["k"][0, 0] == F(16)
    # a plain temporal call's history given to a moments call, and the reverse: no pixel takes history
    plain = TT.denoise(*wall(rs, h, w, cam, n=8), None, cam)[2]
    plain["raw_cam"] = base["raw_cam"]
    _, n_out, _, _ = check(driver, wall(rs, h, w, cam), plain, cam)
    assert (n_out == F(1)).all() and MT.history_for(plain, True) is None and MT.history_for(plain, False) is plain
    call = wall(rs, h, w, cam, n=8)
    assert MT.history_for(base, False) is None and MT.history_for(base, True) is base
    out, n_out, _ = TT.denoise(*call, MT.history_for(base, False), cam)
    assert (n_out == F(8)).all() and differing(out, D.denoise(*call)) == 0


def test_the_new_symbols_are_declared_and_bound():
    import ctypes
    from adypt_amd import _native as N
    header = open(os.path.join(ROOT, "include", "adypt_hip.h")).read()
    for stem in ("denoise_temporal_moments", "read_denoise_variance", "get_denoise_moments"):
        for name in ("adypt_" + stem, "adypt_multi_" + stem):
            assert re.search(r"\bint %s\(" % name, header), name
            assert name in N.EXPORTS and hasattr(N.lib, name), name
    assert "typedef struct adypt_denoise_moments" in header and N.lib.adypt_abi_version() == 4
    assert ctypes.sizeof(N.DenoiseMoments) == 24
    from adypt_amd import api
    for cls in (api.HipPathTracer, api.MultiPathTracer):
        assert hasattr(cls, "ReadDenoiseVariance") and hasattr(cls, "GetDenoiseMoments")


# ---- the edge inputs the kernels are probed with on the GPU (tests/moments_edge_inputs.py), through the header ----
RAW_DRIVER = r"""
#include "temporal.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace adypt;
// IN:  int32 mode, w, h, flag_a, flag_b, then by mode (n = w h; an image is n float4):
//   0  prepare   flag_a: moments_prepare, else denoise_prepare.  float32 C[n][3], m2[n], count[n], A[n][3]                      OUT: X0
//   1  merge     flag_a: have, flag_b: motion.  float32 cap, cam[35], images X0 X1 X2 XA H0 H1 H2 HA and with motion XP XN      OUT: merged, float32 n_out[n]
//   2  variance  float32 origin[3], images merged X1 X2 XA                                                                     OUT: float32 V[n], spatial[n] (0 / 1)
struct Img {
	const Dn4 *a, *b, *c, *d;
	Dn4 x0(int i) const { return a[i]; }
	Dn4 x1(int i) const { return b[i]; }
	Dn4 x2(int i) const { return c[i]; }
	Dn4 xa(int i) const { return d[i]; }
	Dn4 h0(int i) const { return a[i]; }
	Dn4 h1(int i) const { return b[i]; }
	Dn4 h2(int i) const { return c[i]; }
	Dn4 ha(int i) const { return d[i]; }
};
static bool rd(FILE *f, std::vector<float> &v) { return fread(v.data(), 4, v.size(), f) == v.size(); }
static bool image(FILE *f, std::vector<Dn4> &v)
{
	static_assert(sizeof(Dn4) == 16, "four floats");
	return fread(v.data(), 16, v.size(), f) == v.size();
}
int main(int argc, char **argv)
{
	if(argc != 3) return 2;
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if(!in || !out) return 3;
	int32_t h[5];
	if(fread(h, 4, 5, in) != 5) return 4;
	const int width = h[1], height = h[2];
	const size_t n = (size_t)width * height;
	if(h[0] == 0)
	{
		std::vector<float> C(n * 3), m2(n), cnt(n), A(n * 3);
		if(!rd(in, C) || !rd(in, m2) || !rd(in, cnt) || !rd(in, A)) return 4;
		std::vector<Dn4> x0(n);
		for(size_t i = 0; i < n; ++i)
			x0[i] = h[3] ? moments_prepare(C[3 * i], C[3 * i + 1], C[3 * i + 2], m2[i], cnt[i], A[3 * i], A[3 * i + 1], A[3 * i + 2])
			             : denoise_prepare(C[3 * i], C[3 * i + 1], C[3 * i + 2], m2[i], cnt[i], A[3 * i], A[3 * i + 1], A[3 * i + 2]);
		fwrite(x0.data(), 16, n, out);
	}
	else if(h[0] == 1)
	{
		std::vector<float> s(36);
		std::vector<Dn4> x0(n), x1(n), x2(n), xa(n), h0(n), h1(n), h2(n), ha(n), xp(n), xn(n), merged(n);
		if(!rd(in, s) || !image(in, x0) || !image(in, x1) || !image(in, x2) || !image(in, xa) || !image(in, h0) || !image(in, h1) || !image(in, h2) || !image(in, ha)) return 4;
		if(h[4] && (!image(in, xp) || !image(in, xn))) return 4;
		const TemporalCamera tc = temporal_camera(&s[1], &s[4], &s[20]);
		const Img hist{h0.data(), h1.data(), h2.data(), ha.data()};
		std::vector<float> no(n);
		for(size_t i = 0; i < n; ++i)
		{
			const TemporalOut m = h[4] ? temporal_merge_motion<true>(hist, h[3] != 0, tc, width, height, x0[i], x1[i], xa[i], x2[i].w, s[0], xp[i], xn[i])
			                           : temporal_merge<true>(hist, h[3] != 0, tc, width, height, x0[i], x1[i], x2[i], xa[i], x2[i].w, s[0]);
			merged[i] = m.x0; no[i] = m.n;
		}
		fwrite(merged.data(), 16, n, out); fwrite(no.data(), 4, n, out);
	}
	else
	{
		std::vector<float> o(3), V(n), sp(n);
		std::vector<Dn4> x0(n), x1(n), x2(n), xa(n);
		if(!rd(in, o) || !image(in, x0) || !image(in, x1) || !image(in, x2) || !image(in, xa)) return 4;
		const Img img{x0.data(), x1.data(), x2.data(), xa.data()};
		for(int y = 0; y < height; ++y)
			for(int x = 0; x < width; ++x)
			{
				const MomentsVariance r = moments_variance(img, width, height, x, y, o.data());
				V[(size_t)y * width + x] = r.v; sp[(size_t)y * width + x] = r.spatial ? 1.0f : 0.0f;
			}
		fwrite(V.data(), 4, n, out); fwrite(sp.data(), 4, n, out);
	}
	fclose(out);
	return 0;
}
"""


def test_the_probes_edge_inputs_through_the_header(tmp_path):
    """tests/moments_edge_inputs.py — what tests/test_gpu_moments_probes.py gives the kernels — through moments_prepare, denoise_prepare,
    temporal_merge<true>, temporal_merge_motion<true> and moments_variance compiled on the host: header and numpy agree to the bit, and every case reaches
    what it is named after.  The GPU run then adds only kernel against truth."""
    from tests import denoise_edge_inputs as E
    from tests import moments_edge_inputs as M
    src, exe = str(tmp_path / "raw.cpp"), str(tmp_path / "raw")
    open(src, "w").write(RAW_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", DEVICE, src, "-o", exe])

    def run(head, *arrays):
        with open(str(tmp_path / "in.bin"), "wb") as f:
            f.write(np.array(head, np.int32).tobytes() + b"".join(np.ascontiguousarray(a, dtype=np.float32).tobytes() for a in arrays))
        subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        return np.fromfile(str(tmp_path / "out.bin"), dtype=np.float32)

    def agree(got, want, what):
        assert M.same_bits(got, want).all(), "%s: %d words differ from the numpy restatement" % (what, int((~M.same_bits(got, want)).sum()))
    for name, case in M.prepare_cases().items():
        w, h = case["w"], case["h"]
        for instance in ("class", "moments", "virtual"):
            assert M.prepare_reach(case, instance), (name, instance)
        for instance in ("class", "moments"):
            got = run([0, w, h, instance == "moments", 0], case["C"], case["m2"], D.block_counts(h, w, case["spp"]), case["A"])
            agree(got.reshape(h, w, 4), M.prepare_truth(case, instance)[0], "prepare %s %s" % (instance, name))
    for key, case in M.merge_cases().items():
        assert case["reach"](M.merge_truth(case)), key
        im = E.images(case["call"])
        h, w = im["hit"].shape
        hist = case["hist"]
        H, raw = E.h_images(hist if hist is not None else case.get("stale"), h, w)
        _, XP, XN, _ = M.merge_through(case)
        for motion in (False, True):
            t = M.merge_truth(dict((k, v) for k, v in case.items() if motion or k != "tri"), motion=motion)
            got = run([1, w, h, hist is not None, motion], [case["kw"].get("cap", 64.0)], *raw, *E.x_images(im), *H, *((XP, XN) if motion else ()))
            agree(got[:4 * h * w].reshape(h, w, 4), E.rgba(t["D"], t["V"]), "merge %s, motion %s" % (key, motion))
            agree(got[4 * h * w:].reshape(h, w), t["n_out"], "n_out of %s, motion %s" % (key, motion))
    for name, case in M.variance_cases().items():
        t = M.variance_truth(case)
        assert case["reach"](t), name
        w, h = case["w"], case["h"]
        got = run([2, w, h, 0, 0], case["origin"], *M.variance_images(case))
        agree(got[:h * w].reshape(h, w), t["V"], "variance " + name)
        assert np.array_equal(got[h * w:].reshape(h, w) != 0, t["spatial"]), name
