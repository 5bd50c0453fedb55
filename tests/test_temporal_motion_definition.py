"""Following moved geometry through the temporal merge: temporal_previous_point and temporal_merge_motion of csrc/device/temporal.hpp compiled on
the host and held bit for bit against their numpy float32 restatement (tests/temporal_motion_truth.py) on hand-made 16 x 12 images and a handful of
triangles: unmoved, translated, rotated past the normal test, skinned, sky, strangers, a degenerate normal, a NaN vertex, a previous point behind the
history's camera and one that reprojects outside the image.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import denoise_truth as D
from tests import temporal_motion_truth as TM
from tests import temporal_truth as TT
from tests.test_temporal_definition import camera_of, cast, differing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
F = np.float32
W, H, SPP = 16, 12, 8

DRIVER = r"""
#include "temporal.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace adypt;
// IN:  int32 w, h, levels, have, n_prev, n_cur; float32 sigma_l, sigma_z, cap;
//      the call:    float32 C[h][w][3], m2[h][w], n[h][w], A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
//      the history: float32 origin[3], inv_proj[16], inv_view[16], D[h][w][3], V[h][w], n[h][w], A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
//      the motion:  int32 tri[h][w]; float32 uv[h][w][2], prev[n_prev][18], cur[n_cur][18]
// OUT: float32 Dm[h][w][3], Vm[h][w], n_out[h][w], rgb[h][w][3], XP[h][w][4], XN[h][w][4], then Dm, Vm, n_out of temporal_merge (no motion)
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
	int32_t h[6]; float s[3];
	if(fread(h, 4, 6, in) != 6 || fread(s, 4, 3, in) != 3) return 4;
	const int width = h[0], height = h[1];
	const bool have = h[3] != 0;
	const int32_t n_prev = h[4], n_cur = h[5];
	const size_t n = (size_t)width * height;
	std::vector<float> C(n * 3), m2(n), cnt(n), A(n * 3), N(n * 3), P(n * 3), cam(35), hD(n * 3), hV(n), hn(n), hA(n * 3), hN(n * 3), hP(n * 3);
	std::vector<uint8_t> hit(n), hhit(n);
	if(!rd(in, C) || !rd(in, m2) || !rd(in, cnt) || !rd(in, A) || !rd(in, N) || !rd(in, P) || fread(hit.data(), 1, n, in) != n) return 4;
	if(!rd(in, cam) || !rd(in, hD) || !rd(in, hV) || !rd(in, hn) || !rd(in, hA) || !rd(in, hN) || !rd(in, hP) || fread(hhit.data(), 1, n, in) != n) return 4;
	std::vector<int32_t> tri(n);
	std::vector<float> uv(n * 2), prev((size_t)n_prev * kTemporalTriWords), cur((size_t)n_cur * kTemporalTriWords);
	if(fread(tri.data(), 4, n, in) != n || !rd(in, uv) || !rd(in, prev) || !rd(in, cur)) return 4;
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
	std::vector<float> Dm(n * 3), Vm(n), no(n), XP(n * 4), XN(n * 4), pD(n * 3), pV(n), pn(n);
	for(size_t i = 0; i < n; ++i)
	{
		// (an index outside the snapshot is never used as one)
		const bool known = hit[i] && tri[i] >= 0 && tri[i] < n_prev && tri[i] < n_cur;
		const size_t at = known ? (size_t)tri[i] * kTemporalTriWords : 0;
		const TemporalPrevious q = temporal_previous_point(known ? &prev[at] : nullptr, known ? &cur[at] : nullptr, known, uv[2 * i], uv[2 * i + 1], x1[i], x2[i]);
		const TemporalOut m = temporal_merge_motion(hist, have, tc, width, height, x0[i], x1[i], xa[i], x2[i].w, s[2], q.xp, q.xn);
		const TemporalOut p = temporal_merge(hist, have, tc, width, height, x0[i], x1[i], x2[i], xa[i], x2[i].w, s[2]);
		x0b[i] = m.x0; no[i] = m.n;
		Dm[3 * i] = m.x0.x; Dm[3 * i + 1] = m.x0.y; Dm[3 * i + 2] = m.x0.z; Vm[i] = m.x0.w;
		pD[3 * i] = p.x0.x; pD[3 * i + 1] = p.x0.y; pD[3 * i + 2] = p.x0.z; pV[i] = p.x0.w; pn[i] = p.n;
		XP[4 * i] = q.xp.x; XP[4 * i + 1] = q.xp.y; XP[4 * i + 2] = q.xp.z; XP[4 * i + 3] = q.xp.w;
		XN[4 * i] = q.xn.x; XN[4 * i + 1] = q.xn.y; XN[4 * i + 2] = q.xn.z; XN[4 * i + 3] = q.xn.w;
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
	for(const std::vector<float> *v : {&Dm, &Vm, &no, &rgb, &XP, &XN, &pD, &pV, &pn}) fwrite(v->data(), 4, v->size(), out);
	fclose(out);
	return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("temporal_motion_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", DEVICE, src, "-o", exe])
    return exe, str(d)


def run_driver(driver, call, hist, tri, uv, cur, cap=64.0, levels=5, sigma_l=4.0, sigma_z=0.1):
    exe, d = driver
    C, m2, n, A, N, P, hit = call
    h, w = np.shape(m2)
    n = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(h, w, n)
    prev = np.zeros((0, TM.TRI_WORDS), np.float32) if hist is None or hist.get("tris") is None else hist["tris"]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).tobytes()  # noqa: E731
    u8 = lambda a: np.ascontiguousarray(a).astype(np.uint8).tobytes()  # noqa: E731
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([w, h, levels, 0 if hist is None else 1, len(prev), len(cur)], np.int32).tobytes() + np.array([sigma_l, sigma_z, cap], np.float32).tobytes())
        f.write(b"".join(f32(a) for a in (C, m2, n, A, N, P)) + u8(hit))
        if hist is None:
            f.write(bytes(4 * 35 + (3 + 1 + 1 + 3 + 3 + 3) * 4 * h * w + h * w))
        else:
            f.write(f32(hist["raw_cam"]) + b"".join(f32(hist[k]) for k in ("D", "V", "n", "A", "N", "P")) + u8(hist["hit"]))
        f.write(np.ascontiguousarray(tri, dtype=np.int32).tobytes() + f32(uv) + f32(prev) + f32(cur))
    subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    o = np.fromfile(os.path.join(d, "out.bin"), dtype=np.float32)
    k = h * w
    sizes = [("Dm", 3), ("Vm", 1), ("n", 1), ("rgb", 3), ("XP", 4), ("XN", 4), ("plain_D", 3), ("plain_V", 1), ("plain_n", 1)]
    out, at = {}, 0
    for name, c in sizes:
        out[name] = o[at:at + c * k].reshape((h, w, c) if c > 1 else (h, w))
        at += c * k
    assert at == len(o)
    return out


def check(driver, call, hist, cam, tri, uv, cur, **kw):
    """The header and numpy on one motion call: zero differing words in the merged image, the history length, the result and the previous point.
    Returns the driver's output and numpy's (n_out, history the call would commit, motion)."""
    got = run_driver(driver, call, hist, tri, uv, cur, **kw)
    want, want_n, new, motion = TM.denoise(*call, hist, cam, tri, uv, cur, **kw)
    pairs = (("merged D", got["Dm"], new["D"]), ("merged V", got["Vm"], new["V"]), ("history length", got["n"], want_n), ("result", got["rgb"], want),
             ("previous position", got["XP"][..., :3], motion["previous_position"]), ("previous normal", got["XN"][..., :3], motion["previous_normal"]),
             ("moved", got["XP"][..., 3], motion["moved"].astype(np.float32)), ("valid", got["XN"][..., 3], motion["valid"].astype(np.float32)))
    for name, a, b in pairs:
        assert differing(a, b) == 0, "%s: %d words differ from the numpy restatement (%s)" % (name, differing(a, b), kw)
    # temporal_merge beside it, against the truth the existing tests use
    C, m2, n, A, N, P, hit = call
    n2 = np.asarray(n, np.float32) if np.ndim(n) == 2 else D.block_counts(*np.shape(m2), n)
    D0, V0, _ = D.prepare(np.asarray(C, np.float32), m2, n2, np.asarray(A, np.float32))
    pD, pV, pn = TT.merge(D0, V0, n2, np.asarray(N, np.float32), np.asarray(P, np.float32), np.asarray(A, np.float32), hit, hist, kw.get("cap", 64.0))
    assert differing(got["plain_D"], pD) == 0 and differing(got["plain_V"], pV) == 0 and differing(got["plain_n"], pn) == 0, "temporal_merge moved"
    new["raw_cam"] = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in cam])
    return got, want_n, new, motion


def test_header_needs_no_hip_include_and_has_no_fma_exp_or_pow():
    text = open(os.path.join(DEVICE, "temporal.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in "".join(l for l in code.splitlines() if l.startswith("#include")).lower()
    assert not re.search(r"\b(fmaf?|expf?|exp2f?|powf?|__builtin\w*)\b", code)
    assert "temporal_previous_point" in code and "temporal_merge_motion" in code


# ---- the scene: a wall 5 in front of the history's camera, made of one big triangle per index; the call looks at points of it at fractional pixels ----
UNMOVED, TRANSLATED, ROTATED, SKINNED, FLAT_NORMAL, NAN_VERTEX, BEHIND, OUTSIDE = range(8)
N_TRIS = 8


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def scene():
    """(the committed call and its camera, the later call, tri, uv, prev words, cur words, the region of every pixel)."""
    rs = np.random.RandomState(5)
    cam = camera_of(w=W, h=H)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    # the history: the wall at the pixel centres
    Ph, Nh = cast(cam, W, H, xx, yy, 5.0)
    before = [rs.uniform(0, 2, size=(H, W, 3)).astype(np.float32), rs.uniform(0, 3, size=(H, W)).astype(np.float32), SPP, np.full((H, W, 3), 0.5, np.float32), Nh, Ph,
              np.ones((H, W), bool)]
    # the points the later call hits, where the history's camera saw them: a third of a pixel off the centres
    Q, Nq = cast(cam, W, H, xx + 0.3, yy + 0.4, 5.0)
    corners = np.stack([cast(cam, W, H, fx, fy, 5.0)[0] for fx, fy in ((-40.0, -30.0), (60.0, -30.0), (8.0, 80.0))]).astype(np.float64)  # p0 p1 p2
    normal = Nq[0, 0].astype(np.float64)
    right = (corners[1] - corners[0]) / np.linalg.norm(corners[1] - corners[0])
    # (u, v): Q = u p0 + v p1 + (1 - u - v) p2, least squares in float64, rounded once
    M = np.stack([corners[0] - corners[2], corners[1] - corners[2]], 1)
    sol = np.linalg.lstsq(M, (Q.reshape(-1, 3).astype(np.float64) - corners[2]).T, rcond=None)[0].T
    uv = sol.reshape(H, W, 2).astype(np.float32)
    base_p, base_n = corners.copy(), np.tile(normal, (3, 1))
    prev_p, prev_n = np.tile(base_p, (N_TRIS, 1, 1)), np.tile(base_n, (N_TRIS, 1, 1))
    cur_p, cur_n = prev_p.copy(), prev_n.copy()
    cur_p[TRANSLATED] += np.array([1.0, -0.5, 0.75])  # ten times the plane tolerance (0.02 x 5)
    R = rotation(np.cross(normal, right), 60.0)  # turns the normal by 60 degrees: past acos 0.9 = 25.8
    centre = base_p.mean(0)
    cur_p[ROTATED] = (base_p - centre) @ R.T + centre + np.array([0.2, 0.1, -0.3])
    cur_n[ROTATED] = base_n @ R.T
    cur_p[SKINNED] += np.array([[0.5, 0.0, 0.0], [0.0, 0.8, -0.2], [-0.3, 0.1, 0.6]])  # every vertex its own way
    cur_n[SKINNED] = base_n + np.array([[0.3, 0.0, 0.0], [0.0, 0.2, 0.0], [0.0, 0.0, -0.4]])
    prev_n[FLAT_NORMAL] = 0.0  # the previous normals combine to length 0
    cur_p[FLAT_NORMAL] += 0.01
    prev_p[NAN_VERTEX, 1, 2] = np.nan
    prev_p[BEHIND] = base_p + 10.0 * normal  # the wall's normal looks at the camera, 5 away: 10 along it is behind it
    prev_p[OUTSIDE] = base_p + 50.0 * right
    prev, cur = TM.tri_words(prev_p, prev_n), TM.tri_words(cur_p, cur_n)
    region = np.zeros((H, W), np.int32)
    for x, r in enumerate((0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, -1, -2, 6)):
        region[:, x] = r
    region[6:, 15] = OUTSIDE
    tri = region.copy()
    tri[:6, 14], tri[6:9, 14], tri[9:, 14] = N_TRIS, 2 ** 31 - 1, -7  # strangers: ids the snapshot does not hold
    hit = region != -1  # column 13 is sky
    # what the later call sees: the hit's combination of the triangle as it is now (any float32 will do as an input; strangers and sky: the wall)
    t = np.where((tri >= 0) & (tri < N_TRIS), tri, 0)
    u, v = uv[..., 0:1].astype(np.float64), uv[..., 1:2].astype(np.float64)
    P = (cur_p[t][..., 0, :] * u + cur_p[t][..., 1, :] * v + cur_p[t][..., 2, :] * (1 - u - v)).astype(np.float32)
    Nn = cur_n[t][..., 0, :] * u + cur_n[t][..., 1, :] * v + cur_n[t][..., 2, :] * (1 - u - v)
    Nn = (Nn / np.linalg.norm(Nn, axis=-1, keepdims=True)).astype(np.float32)
    P[~hit], Nn[~hit] = 0, 0
    after = [rs.uniform(0, 2, size=(H, W, 3)).astype(np.float32), rs.uniform(0, 3, size=(H, W)).astype(np.float32), SPP, np.full((H, W, 3), 0.5, np.float32), Nn, P, hit]
    after[3][~hit] = 0
    return before, cam, after, tri, uv, prev, cur, region


def test_moved_triangles_find_their_history_bit_for_bit(driver):
    before, cam, after, tri, uv, prev, cur, region = scene()
    n = F(SPP)
    # the committing motion call: no history yet, the plain filter's bits, and it leaves the snapshot
    got, want_n, hist, motion = check(driver, before, None, cam, tri, uv, prev)
    assert (want_n == n).all() and not motion["moved"].any() and differing(got["rgb"], D.denoise(*before)) == 0
    assert differing(hist["tris"], prev) == 0
    for kw in ({}, {"cap": 3.0}, {"levels": 2, "sigma_l": 2.0, "sigma_z": 0.3}):
        got, want_n, _, motion = check(driver, after, hist, cam, tri, uv, cur, **kw)
    got, want_n, _, motion = check(driver, after, hist, cam, tri, uv, cur)
    plain_n = got["plain_n"]
    inner = np.zeros((H, W), bool)
    inner[:-1, :-1] = True  # (the last row and column reproject onto the border: some taps lie outside)
    moved, valid = motion["moved"], motion["valid"]
    assert np.array_equal(moved, (region >= TRANSLATED) & (tri == region)), "moved is not exactly the pixels on a triangle whose words changed"
    for r, name in ((TRANSLATED, "translated"), (ROTATED, "rotated"), (SKINNED, "skinned")):
        at = (region == r) & inner
        assert at.sum() >= 10 and (want_n[at] > n).all(), name + ": the motion merge found no history"
        assert (plain_n[at] == n).all(), name + ": the case does not refuse the plain merge"
        assert valid[at].all()
    # the previous point is the wall point the history's camera saw a third of a pixel off the centre
    ok, fx, fy, _ = TT.reproject(hist["cam"], W, H, motion["previous_position"])
    yy, xx = np.mgrid[0:H, 0:W]
    at = np.isin(region, (TRANSLATED, ROTATED, SKINNED))
    assert ok[at].all() and np.abs(fx - (xx + 0.3))[at].max() < 0.02 and np.abs(fy - (yy + 0.4))[at].max() < 0.02
    # unmoved, strangers and sky: temporal_merge's bits; the first two take history, sky none
    same = ~moved
    assert differing(got["Dm"][same], got["plain_D"][same]) == 0 and differing(got["Vm"][same], got["plain_V"][same]) == 0 and differing(want_n[same], plain_n[same]) == 0
    assert differing(motion["previous_position"][same], after[5][same]) == 0 and differing(motion["previous_normal"][same], after[4][same]) == 0
    assert (want_n[(region == UNMOVED) & inner] > n).all() and (want_n[(region == -2) & inner] > n).all() and (want_n[region == -1] == n).all()
    # a zero-length previous normal: not valid, no history; a NaN vertex, a point behind the camera, a point outside the image: valid or not, no history
    assert not valid[region == FLAT_NORMAL].any() and (motion["previous_normal"][region == FLAT_NORMAL] == 0).all()
    for r in (FLAT_NORMAL, NAN_VERTEX, BEHIND, OUTSIDE):
        assert moved[region == r].all() and (want_n[region == r] == n).all(), r
    assert np.isnan(motion["previous_position"][region == NAN_VERTEX]).any(-1).all()
    assert not ok[region == BEHIND].any() and ok[region == OUTSIDE].all() and (fx[region == OUTSIDE] >= W).all()
    assert np.isfinite(got["Dm"]).all() and np.isfinite(got["Vm"]).all() and np.isfinite(got["n"]).all()


def test_every_triangle_unmoved_is_temporal_merge_bit_for_bit(driver):
    before, cam, after, tri, uv, prev, cur, region = scene()
    _, _, hist, _ = check(driver, before, None, cam, tri, uv, prev)
    # the wall as it was: what the later call sees is the previous point itself
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    Qp, Qn = cast(cam, W, H, xx + 0.3, yy + 0.4, 5.0)
    still = list(after)
    still[5], still[4] = Qp.copy(), Qn.copy()
    still[5][~after[6]], still[4][~after[6]] = 0, 0
    inner = after[6].copy()
    inner[-1, :], inner[:, -1] = False, False
    cases = {"the records are the snapshot's (a NaN word included)": (hist, prev.copy()),
             "no snapshot: a history a plain call committed": ({k: v for k, v in hist.items() if k != "tris"}, cur),
             "an empty snapshot": (dict(hist, tris=np.zeros((0, TM.TRI_WORDS), np.float32)), cur)}
    for name, (h, now) in cases.items():
        got, want_n, _, motion = check(driver, still, h, cam, tri, uv, now)
        assert not motion["moved"].any() and motion["valid"].all(), name
        assert differing(got["Dm"], got["plain_D"]) == 0 and differing(got["Vm"], got["plain_V"]) == 0 and differing(got["n"], got["plain_n"]) == 0, name
        assert (want_n[inner] > F(SPP)).all(), name
    # the words are compared as bits: -0.0 against 0.0 is a moved triangle (whose previous point is the same point)
    zero, minus = prev.copy(), prev.copy()
    zero[:, 2], minus[:, 2] = 0.0, -0.0
    _, _, _, motion = check(driver, still, dict(hist, tris=zero), cam, tri, uv, minus)
    assert motion["moved"][(region >= 0) & (tri == region)].all() and not motion["moved"][region < 0].any()


def test_the_new_symbols_are_declared_and_bound():
    from adypt_amd import _native as N
    import ctypes
    header = open(os.path.join(ROOT, "include", "adypt_hip.h")).read()
    for stem in ("denoise_temporal_motion", "read_denoise_motion", "get_denoise_motion"):
        for name in ("adypt_" + stem, "adypt_multi_" + stem):
            assert re.search(r"\bint %s\(" % name, header), name
            assert name in N.EXPORTS and hasattr(N.lib, name), name
    assert "typedef struct adypt_denoise_motion" in header and N.lib.adypt_abi_version() == 4
    assert ctypes.sizeof(N.TemporalParams) == 8  # (adypt_temporal_params is ABI: the motion call is a call of its own)
    assert ctypes.sizeof(N.DenoiseMotion) == 24


def test_the_named_edge_inputs(driver):
    """tests/denoise_edge_inputs.py's entries for the motion form of the merge — no history, moved triangles, XN.w = 0, records that did not change, a
    history without a snapshot — each reaching its branch by the truth's account: zero differing words."""
    from tests import denoise_edge_inputs as E  # (here: the module imports this file's generators)
    for name, case in E.motion_cases().items():
        assert case["reach"](E.motion_truth(case)), name + ": the case does not reach what it is named after"
        try:
            check(driver, case["call"], case["hist"], case["cam"], case["tri"], case["uv"], case["cur"], **case["kw"])
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
