"""The temporal merge's definition (csrc/device/temporal.hpp) compiled on the host and held bit for bit against its numpy float32 restatement
(tests/temporal_truth.py): on sequences of cameras whose images, moments and guides the CPU oracle makes, and on hand-made edge cases.  Its quality is
measured against the oracle's converged image at the last camera, never against the code under test.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import denoise_truth as D
from tests import noise_truth as T
from tests import temporal_truth as TT
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
// IN:  int32 w, h, levels, have; float32 sigma_l, sigma_z, cap;
//      the call:    float32 C[h][w][3], m2[h][w], n[h][w], A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
//      the history: float32 origin[3], inv_proj[16], inv_view[16], D[h][w][3], V[h][w], n[h][w], A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
// OUT: float32 Dm[h][w][3], Vm[h][w], n_out[h][w], rgb[h][w][3]
struct Img {
	const Dn4 *a, *b, *c;
	Dn4 x0(int i) const { return a[i]; }
	Dn4 x1(int i) const { return b[i]; }
	Dn4 x2(int i) const { return c[i]; }
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
	int32_t h[4]; float s[3];
	if(fread(h, 4, 4, in) != 4 || fread(s, 4, 3, in) != 3) return 4;
	const int width = h[0], height = h[1];
	const bool have = h[3] != 0;
	const size_t n = (size_t)width * height;
	std::vector<float> C(n * 3), m2(n), cnt(n), A(n * 3), N(n * 3), P(n * 3), cam(35), hD(n * 3), hV(n), hn(n), hA(n * 3), hN(n * 3), hP(n * 3);
	std::vector<uint8_t> hit(n), hhit(n);
	if(!rd(in, C) || !rd(in, m2) || !rd(in, cnt) || !rd(in, A) || !rd(in, N) || !rd(in, P) || fread(hit.data(), 1, n, in) != n) return 4;
	if(!rd(in, cam) || !rd(in, hD) || !rd(in, hV) || !rd(in, hn) || !rd(in, hA) || !rd(in, hN) || !rd(in, hP) || fread(hhit.data(), 1, n, in) != n) return 4;
	const DenoiseParams prm{h[2], s[0], s[1]};
	if(!denoise_params_valid(prm) || !temporal_cap_valid(s[2])) return 5;
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
	std::vector<float> Dm(n * 3), Vm(n), no(n);
	for(int y = 0; y < height; ++y)
		for(int x = 0; x < width; ++x)
		{
			const size_t i = (size_t)y * width + x;
			const TemporalOut m = temporal_merge(hist, have, tc, width, height, x0[i], x1[i], x2[i], xa[i], x2[i].w, s[2]);
			x0b[i] = m.x0; no[i] = m.n;
			Dm[3 * i] = m.x0.x; Dm[3 * i + 1] = m.x0.y; Dm[3 * i + 2] = m.x0.z; Vm[i] = m.x0.w;
		}
	x0.swap(x0b);
	for(int l = 0; l < prm.levels; ++l)
	{
		const Img img{x0.data(), x1.data(), x2.data()};
		for(int y = 0; y < height; ++y)
			for(int x = 0; x < width; ++x) x0b[(size_t)y * width + x] = denoise_level(img, width, height, x, y, 1 << l, prm.sigma_l, prm.sigma_z);
		x0.swap(x0b);
	}
	std::vector<float> rgb(n * 3);
	for(size_t i = 0; i < n; ++i) denoise_remodulate(x0[i], xa[i], &rgb[3 * i]);
	fwrite(Dm.data(), 4, Dm.size(), out); fwrite(Vm.data(), 4, Vm.size(), out); fwrite(no.data(), 4, no.size(), out); fwrite(rgb.data(), 4, rgb.size(), out);
	fclose(out);
	return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("temporal_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", DEVICE, src, "-o", exe])
    return exe, str(d)


def run_driver(driver, call, hist, cap=64.0, levels=5, sigma_l=4.0, sigma_z=0.1):
    """One temporal call of the header: (Dm, Vm, n_out, rgb).  call = (C, m2, n, A, N, P, hit), hist = what TT.commit makes, or None."""
    exe, d = driver
    C, m2, n, A, N, P, hit = call
    h, w = np.shape(m2)
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).tobytes()  # noqa: E731
    u8 = lambda a: np.ascontiguousarray(a).astype(np.uint8).tobytes()  # noqa: E731
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([w, h, levels, 0 if hist is None else 1], np.int32).tobytes() + np.array([sigma_l, sigma_z, cap], np.float32).tobytes())
        f.write(b"".join(f32(a) for a in (C, m2, n, A, N, P)) + u8(hit))
        if hist is None:
            f.write(bytes(4 * 35 + (3 + 1 + 1 + 3 + 3 + 3) * 4 * h * w + h * w))
        else:
            f.write(f32(hist["raw_cam"]) + b"".join(f32(hist[k]) for k in ("D", "V", "n", "A", "N", "P")) + u8(hist["hit"]))
    subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    o = np.fromfile(os.path.join(d, "out.bin"), dtype=np.float32)
    k = h * w
    return o[:3 * k].reshape(h, w, 3), o[3 * k:4 * k].reshape(h, w), o[4 * k:5 * k].reshape(h, w), o[5 * k:].reshape(h, w, 3)


def differing(a, b):
    return int((bits(np.ascontiguousarray(a, np.float32)) != bits(np.ascontiguousarray(b, np.float32))).sum())


def check(driver, call, hist, cam, **kw):
    """The header and numpy on one call: zero differing words in the merged image, the history length and the result.  Returns numpy's
    (result, n_out, history the call would commit)."""
    Dm, Vm, no, rgb = run_driver(driver, call, hist, **kw)
    want, want_n, new = TT.denoise(*call, hist, cam, **kw)
    for name, got, exp in (("merged D", Dm, new["D"]), ("merged V", Vm, new["V"]), ("history length", no, want_n), ("result", rgb, want)):
        assert differing(got, exp) == 0, "%s: %d words differ from the numpy restatement (%s)" % (name, differing(got, exp), kw)
    new["raw_cam"] = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in cam])
    return want, want_n, new


def test_header_needs_no_hip_include_and_has_no_fma_exp_or_pow():
    text = open(os.path.join(DEVICE, "temporal.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in "".join(l for l in code.splitlines() if l.startswith("#include")).lower()
    assert not re.search(r"\b(fmaf?|expf?|exp2f?|powf?|__builtin\w*)\b", code)
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", DEVICE, "-x", "c++", "-"],
                   input=b'#include "temporal.hpp"\nint main() { return adypt::temporal_cap_valid(adypt::kTemporalDefaultCap) ? 0 : 1; }\n', check=True)


# ---- sequences of cameras, everything made by the CPU oracle ----
# A step of the camera: 1.5 degrees of yaw and 0.15 scene units along one axis — a slow orbit, a few pixels of motion per pose at these sizes, so that
# neighbouring poses see mostly the same surfaces (the situation the feature is for) while every pixel reprojects to a fractional position.
STEP_YAW, STEP_MOVE = 1.5, 0.15
SEQUENCES = {"sibenik": ("sibenik", 96, 54, 3, 2), "tiny0": ("tiny0", 100, 75, 16, 0)}  # name, W, H, tmpLifetime, the axis the camera moves along
_sequence = {}


def oracle_sequence(scene_cache, sobol_matrices, key, n_cameras=4, spp=4):
    """[(call inputs, (origin, inv_proj, inv_view))] of the cameras, and the oracle's 1024-spp image at the last; once per scene."""
    if key in _sequence:
        return _sequence[key]
    from adypt_amd import api, scenes
    name, w, h, life, axis = SEQUENCES[key]
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
    calls, ref = [], None
    for k in range(n_cameras):
        c.yaw = yaw0 + STEP_YAW * k
        pos = list(pos0)
        pos[axis] += STEP_MOVE * k
        for i in range(3):
            c.position[i] = pos[i]
        P, shift = T.oracle_params(c), O.shift_bytes(SEED + k, w, h)  # a seed of its own per camera
        samples = T.frame_samples(osc, P, shift, sobol_matrices, spp)
        _, m2 = T.moments(samples)
        state = O.PathTracerState(w, h)
        O.pt_frames(osc, P, shift, sobol_matrices, state, spp)
        guides = [O.primary_frame(osc, P, t) for t in (0, 4, 5)]
        hit = guides[0][1]["tri_id"] != -1
        call = (state.accum[..., :3].copy(), m2, spp, guides[0][0][..., :3].copy(), guides[1][0][..., :3].copy(), guides[2][0][..., :3].copy(), hit)
        ip, iv = O.camera(c.fov, c.yaw, c.pitch, w, h)
        calls.append((call, (np.array(pos, np.float32), ip, iv)))
        if k == n_cameras - 1:
            O.pt_frames(osc, P, shift, sobol_matrices, state, 1024 - state.spp)
            ref = state.accum[..., :3].copy()
    _sequence[key] = (calls, ref)
    return _sequence[key]


def run_sequence(driver, calls, cap):
    hist = None
    for call, cam in calls:
        out, n_out, hist = check(driver, call, hist, cam, cap=cap)
    return out, n_out, call


@pytest.mark.parametrize("key", ["sibenik", "tiny0"])
def test_oracle_sequences_are_bit_exact_and_history_helps(key, driver, scene_cache, sobol_matrices):
    """Four cameras a step apart, 4 spp each, a seed per camera, committing; caps 64 and 8.  Header against numpy: zero differing words at every step.
    At the last camera against the oracle's 1024-spp image there: the temporal error is strictly below the spatial-only error, on sibenik at most
    0.85 of it, and at least half of the hit pixels found history.
    Measured, printed by this test and quoted in DESIGN.md section 4, Temporal merge (rmse raw / spatial only / with history, ratio, hit pixels with
    history):   sibenik 96x54   0.5305 / 0.1655 / 0.1111   0.671   95.3 %
                tiny0 100x75    0.5699 / 0.2209 / 0.2011   0.910   99.0 %"""
    calls, ref = oracle_sequence(scene_cache, sobol_matrices, key)
    out, n_out, last = run_sequence(driver, calls, 64.0)
    out8, n_out8, _ = run_sequence(driver, calls, 8.0)
    assert np.isfinite(out).all() and np.isfinite(out8).all()
    hit, n = last[6], F(last[2])
    assert (n_out8 <= n + F(8.0)).all() and (n_out[~hit] == n).all()
    found = float((n_out[hit] > n).mean())
    raw, spatial, temporal, temporal8 = D.rmse(last[0], ref), D.rmse(D.denoise(*last), ref), D.rmse(out, ref), D.rmse(out8, ref)
    print("%s: rmse raw %.4f spatial only %.4f with history %.4f (cap 8: %.4f) history / spatial %.3f, %.1f %% of the hit pixels found history, mean length %.2f"
          % (key, raw, spatial, temporal, temporal8, temporal / spatial, 100.0 * found, float(n_out[hit].mean())))
    assert found >= 0.5
    assert temporal < spatial
    if key == "sibenik":
        assert temporal <= 0.85 * spatial


# ---- hand-made cases ----
def cast(cam, w, h, fx, fy, depth):
    """The world point the camera (origin, inv_proj, inv_view) sees at the continuous pixel coordinates (fx, fy) (pixel centres are the integers) on the
    plane `depth` in front of it, and that plane's normal towards the camera; float64 arithmetic rounded to float32 once."""
    o, m, v = (np.asarray(x, np.float64).reshape(-1) for x in cam)
    sx, sy = (np.asarray(fx, np.float64) + 0.5) * 2.0 / w - 1.0, 1.0 - (np.asarray(fy, np.float64) + 0.5) * 2.0 / h
    t = [m[i] * sx + m[4 + i] * sy + (m[8 + i] + m[12 + i]) for i in range(3)]
    d = [v[i] * t[0] + v[4 + i] * t[1] + v[8 + i] * t[2] for i in range(3)]
    c = np.array([v[i] * (m[8] + m[12]) + v[4 + i] * (m[9] + m[13]) + v[8 + i] * (m[10] + m[14]) for i in range(3)])
    P = np.stack([o[i] + depth * d[i] for i in range(3)], -1).astype(np.float32)
    N = np.broadcast_to((-c / np.linalg.norm(c)).astype(np.float32), P.shape).copy()
    return P, N


def camera_of(yaw=20.0, pitch=-10.0, pos=(1.0, 2.0, 3.0), w=13, h=9):
    ip, iv = O.camera(45.0, yaw, pitch, w, h)
    return (np.array(pos, np.float32), ip, iv)


def wall(rs, h, w, cam, depth=5.0, fx=None, fy=None, n=8, albedo=0.5):
    """The inputs of a call that sees a wall `depth` in front of `cam` (at the pixel centres, or at the coordinates given): random radiance and moments."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    P, N = cast(cam, w, h, xx if fx is None else fx, yy if fy is None else fy, depth)
    C = rs.uniform(0, 2, size=(h, w, 3)).astype(np.float32)
    m2 = rs.uniform(0, 3, size=(h, w)).astype(np.float32)
    A = np.full((h, w, 3), albedo, np.float32)
    return [C, m2, n, A, N, P, np.ones((h, w), bool)]


def history_of(driver, call, cam, **kw):
    return check(driver, call, None, cam, **kw)[2]


def test_hand_made_cases(driver):
    rs = np.random.RandomState(11)
    # the smallest images, the camera unchanged
    for h, w in ((1, 1), (2, 3)):
        cam = camera_of(w=w, h=h)
        hist = history_of(driver, wall(rs, h, w, cam), cam)
        out, n_out, _ = check(driver, wall(rs, h, w, cam), hist, cam)
        assert np.isfinite(out).all() and (n_out > F(8)).all()
    h, w = 9, 13
    cam = camera_of()
    # nothing but sky, now and before
    sky = wall(rs, h, w, cam)
    sky[6][:] = False
    for k in (3, 4, 5):
        sky[k][:] = 0
    hist = history_of(driver, sky, cam)
    out, n_out, _ = check(driver, sky, hist, cam)
    assert np.isfinite(out).all() and (n_out == F(8)).all()
    hist = history_of(driver, wall(rs, h, w, cam), cam)
    # an unchanged camera: every pixel finds its own history; a first call and a call under another cap likewise
    call = wall(rs, h, w, cam)
    out, n_out, _ = check(driver, call, hist, cam)
    assert np.isfinite(out).all() and (n_out > F(15.9)).all() and (n_out < F(16.1)).all()
    # history_cap below n
    out, n_out, _ = check(driver, call, hist, cam, cap=2.0)
    assert (n_out == F(10)).all()
    # the camera turned by 180 degrees: the wall is behind the history's camera, no pixel takes history, the result is the plain filter's bits
    back = camera_of(yaw=200.0)
    turned = history_of(driver, wall(rs, h, w, back), back)
    call = wall(rs, h, w, cam)
    out, n_out, _ = check(driver, call, turned, cam)
    assert (n_out == F(8)).all() and differing(out, D.denoise(*call)) == 0
    # the reprojection on the image border and just outside it, on all four sides
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    edge_x = np.array([-1.5, -1.001, -1.0, -0.999, -0.5, 0.0, 5.25, w - 1.5, w - 1.001, w - 1.0, w - 0.999, w - 0.5, w + 0.5])
    edge_y = np.array([-1.5, -1.0, -0.999, -0.5, 3.75, h - 1.001, h - 1.0, h - 0.5, h + 0.5])
    fx, fy = np.broadcast_to(edge_x[None, :], (h, w)), np.broadcast_to(edge_y[:, None], (h, w))
    call = wall(rs, h, w, cam, fx=fx, fy=fy)
    out, n_out, _ = check(driver, call, hist, cam)
    took = n_out > F(8)
    assert np.isfinite(out).all()
    assert not took[:, 0].any() and not took[:, -1].any() and not took[0, :].any() and not took[-1, :].any(), "a pixel aimed outside the image took history"
    assert took[3:8, 4:12].all(), "a pixel aimed inside the image (or half a pixel outside) took none"
    # NaN in P, in N, and in the history (D, V, n, P, N, A of one pixel each): finite everywhere else, and no NaN spreads through the merge
    call = wall(rs, h, w, cam)
    call[5][2, 3, 1] = np.nan
    call[4][6, 7, 0] = np.nan
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in hist.items()}
    for i, k in enumerate(("D", "V", "n", "P", "N", "A")):
        bad[k][1 + i, 9] = np.nan
    bad["V"][7, 2] = np.inf
    Dm, Vm, no, rgb = run_driver(driver, call, bad)
    want, want_n, new = TT.denoise(*call, bad, cam)
    assert differing(Dm, new["D"]) == 0 and differing(Vm, new["V"]) == 0 and differing(no, want_n) == 0 and differing(rgb, want) == 0
    assert np.isfinite(Dm).all() and np.isfinite(Vm).all() and np.isfinite(no).all()
    assert no[2, 3] == F(8) and no[6, 7] == F(8)
    # a history tap of albedo 0 (an emitter: demodulated by the floor 0.01) next to a lit wall, seen half a pixel to the side: the wall pixel
    # between them refuses the tap — its length is the wall's, not the mean of both — and the result stays the wall's size
    before = wall(rs, h, w, cam)
    before[3][:, 6] = 0
    before[0][:, 6] = 50.0
    before[2] = np.full((h, w), 8, np.float32)
    before[2][:, 6] = 100
    emitter = history_of(driver, before, cam)
    call = wall(rs, h, w, cam, fx=xx + 0.5)
    out, n_out, _ = check(driver, call, emitter, cam)
    assert np.isfinite(out).all() and (n_out[:, 5] < F(16.1)).all() and (n_out[:, 5] > F(15.9)).all() and (n_out[:, 6] < F(16.1)).all()
    assert out[:, 4:8].max() < 10.0  # (radiance below 2 and albedo 0.5; an accepted tap would bring 5000 * 0.51)
    # the plane moved along its normal by less and by more than the tolerance (0.02 of the distance 5)
    for delta, keeps in ((0.05, True), (0.2, False)):
        call = wall(rs, h, w, cam, depth=5.0 - delta)
        out, n_out, _ = check(driver, call, hist, cam)
        assert np.isfinite(out).all()
        assert (n_out[2:-2, 2:-2] > F(8)).all() if keeps else (n_out == F(8)).all(), delta


def test_the_new_symbols_are_declared_and_bound():
    from adypt_amd import _native as N
    header = open(os.path.join(ROOT, "include", "adypt_hip.h")).read()
    for stem in ("denoise_temporal", "denoise_history_reset", "read_denoise_history", "get_denoise_merge_ms"):
        for name in ("adypt_" + stem, "adypt_multi_" + stem):
            assert re.search(r"\bint %s\(" % name, header), name
            assert name in N.EXPORTS and hasattr(N.lib, name), name
    assert "typedef struct adypt_temporal_params" in header and N.lib.adypt_abi_version() == 4
    import ctypes
    assert ctypes.sizeof(N.TemporalParams) == 8 and ctypes.sizeof(N.DenoiseParams) == 12


def test_the_named_edge_inputs(driver):
    """tests/denoise_edge_inputs.py's entries for the merge — the sizes round the 32 x 8 workgroup, every refusal of temporal_merge_through in turn, sw on
    both sides of kTemporalMinWeight — each reaching its branch by the truth's account: zero differing words."""
    from tests import denoise_edge_inputs as E  # (here: the module imports this file's generators)
    for name, case in E.temporal_cases().items():
        assert case["reach"](E.merge_truth(case)), name + ": the case does not reach what it is named after"
        try:
            check(driver, case["call"], case["hist"], case["cam"], **case["kw"])
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
