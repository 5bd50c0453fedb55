"""The definition of history-aware sampling (csrc/device/history_reach.hpp) compiled on the host with -ffp-contract=off and held against its
restatement (tests/history_reach_truth.py) on hand-made histories of 7 x 5 and 37 x 33 pixels: the reach bit for bit, the bins, and the proof against
the merge itself — for the same inputs and any n, the compiled temporal_merge's out.n has the bits of n + reach where the reach is positive and of n
where it is 0; temporal_merge_motion likewise.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import history_reach_truth as HT
from tests import temporal_motion_truth as TM
from tests import temporal_truth as TT
from tests.helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
F = np.float32

DRIVER = r"""
#include "history_reach.hpp"
#include <cstdio>
#include <vector>
using namespace adypt;
// IN:  int32 w, h, have, motion, n_prev, n_cur; float32 cap, n_own;
//      the call:    float32 A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
//      the history: float32 origin[3], inv_proj[16], inv_view[16], D[h][w][3], V[h][w], n[h][w], A[h][w][3], N[h][w][3], P[h][w][3]; uint8 hit[h][w]
//      motion:      int32 tri[h][w]; float32 uv[h][w][2], prev[n_prev][18], cur[n_cur][18]
// OUT: float32 reach[h][w], merged_n[h][w] (temporal_merge's or temporal_merge_motion's out.n for n = n_own); uint32 bins[blocks][65]
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
	int32_t h[6]; float s[2];
	if(fread(h, 4, 6, in) != 6 || fread(s, 4, 2, in) != 2) return 4;
	const int width = h[0], height = h[1];
	const bool have = h[2] != 0, motion = h[3] != 0;
	const size_t n = (size_t)width * height;
	std::vector<float> A(n * 3), N(n * 3), P(n * 3), cam(35), hD(n * 3), hV(n), hn(n), hA(n * 3), hN(n * 3), hP(n * 3), uv(n * 2), prev((size_t)h[4] * 18), cur((size_t)h[5] * 18);
	std::vector<uint8_t> hit(n), hhit(n);
	std::vector<int32_t> tri(n);
	if(!rd(in, A) || !rd(in, N) || !rd(in, P) || fread(hit.data(), 1, n, in) != n) return 4;
	if(!rd(in, cam) || !rd(in, hD) || !rd(in, hV) || !rd(in, hn) || !rd(in, hA) || !rd(in, hN) || !rd(in, hP) || fread(hhit.data(), 1, n, in) != n) return 4;
	if(motion && (fread(tri.data(), 4, n, in) != n || !rd(in, uv) || !rd(in, prev) || !rd(in, cur))) return 4;
	const TemporalCamera tc = temporal_camera(&cam[0], &cam[3], &cam[19]);
	std::vector<Dn4> h0(n), h1(n), h2(n), ha(n);
	for(size_t i = 0; i < n; ++i)
	{
		h0[i] = Dn4{hD[3 * i], hD[3 * i + 1], hD[3 * i + 2], hV[i]};
		h1[i] = Dn4{hN[3 * i], hN[3 * i + 1], hN[3 * i + 2], hhit[i] ? 1.0f : 0.0f};
		h2[i] = Dn4{hP[3 * i], hP[3 * i + 1], hP[3 * i + 2], hn[i]};
		ha[i] = Dn4{hA[3 * i], hA[3 * i + 1], hA[3 * i + 2], 0.0f};
	}
	const Hist hist{h0.data(), h1.data(), h2.data(), ha.data()};
	const int nbx = (width + 31) / 32, nby = (height + 31) / 32;
	std::vector<float> reach(n), merged(n);
	std::vector<uint32_t> bins((size_t)nbx * nby * kReachBins, 0u);
	const Dn4 c0{0.25f, 0.5f, 0.75f, 0.125f};
	for(int y = 0; y < height; ++y)
		for(int x = 0; x < width; ++x)
		{
			const size_t i = (size_t)y * width + x;
			const Dn4 c1{N[3 * i], N[3 * i + 1], N[3 * i + 2], hit[i] ? 1.0f : 0.0f}, c2{P[3 * i], P[3 * i + 1], P[3 * i + 2], s[1]}, ca{A[3 * i], A[3 * i + 1], A[3 * i + 2], 0.0f};
			if(motion)
			{
				const int32_t t = tri[i];
				const bool known = t >= 0 && t < h[4] && t < h[5];
				const float zero[18] = {};
				const TemporalPrevious p = temporal_previous_point(known ? &prev[(size_t)t * 18] : zero, known ? &cur[(size_t)t * 18] : zero, known, uv[2 * i], uv[2 * i + 1], c1, c2);
				reach[i] = history_reach_motion(hist, have, tc, width, height, c1, ca, s[0], p.xp, p.xn);
				merged[i] = temporal_merge_motion(hist, have, tc, width, height, c0, c1, ca, s[1], s[0], p.xp, p.xn).n;
			}
			else
			{
				reach[i] = history_reach_still(hist, have, tc, width, height, c1, c2, ca, s[0]);
				merged[i] = temporal_merge(hist, have, tc, width, height, c0, c1, c2, ca, s[1], s[0]).n;
			}
			if(hit[i]) bins[(size_t)((y >> 5) * nbx + (x >> 5)) * kReachBins + reach_bin(reach[i])] += 1u;
		}
	fwrite(reach.data(), 4, n, out); fwrite(merged.data(), 4, n, out); fwrite(bins.data(), 4, bins.size(), out);
	fclose(out);
	return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("history_reach_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", DEVICE, src, "-o", exe])
    return exe, str(d)


def run_driver(driver, call, hist, cap=64.0, n_own=4.0, motion=None):
    """(reach, merged n, bins) of the header.  call = (A, N, P, hit); hist: what TT.commit makes plus raw_cam, or None; motion = (tri, uv, cur)."""
    exe, d = driver
    A, N, P, hit = call
    h, w = np.shape(hit)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).tobytes()  # noqa: E731
    u8 = lambda a: np.ascontiguousarray(a).astype(np.uint8).tobytes()  # noqa: E731
    prev = np.zeros((0, 18), np.float32) if hist is None or hist.get("tris") is None else hist["tris"]
    cur = np.zeros((0, 18), np.float32) if motion is None else np.asarray(motion[2], np.float32).reshape(-1, 18)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([w, h, 0 if hist is None else 1, 0 if motion is None else 1, len(prev), len(cur)], np.int32).tobytes() + np.array([cap, n_own], np.float32).tobytes())
        f.write(b"".join(f32(a) for a in (A, N, P)) + u8(hit))
        if hist is None:
            f.write(bytes(4 * 35 + (3 + 1 + 1 + 3 + 3 + 3) * 4 * h * w + h * w))
        else:
            f.write(f32(hist["raw_cam"]) + b"".join(f32(hist[k]) for k in ("D", "V", "n", "A", "N", "P")) + u8(hist["hit"]))
        if motion is not None:
            f.write(np.ascontiguousarray(motion[0], np.int32).tobytes() + f32(motion[1]) + f32(prev) + f32(cur))
    subprocess.check_call([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    raw = np.fromfile(os.path.join(d, "out.bin"), dtype=np.uint32)
    k = h * w
    return raw[:k].view(np.float32).reshape(h, w), raw[k:2 * k].view(np.float32).reshape(h, w), raw[2 * k:].reshape(-1, HT.BINS)


def same(a, b):
    return np.array_equal(bits(np.ascontiguousarray(a, np.float32)), bits(np.ascontiguousarray(b, np.float32)))


def check(driver, call, hist, cap=64.0, n_values=(2.0, 4.0, 37.0), motion=None):
    """The header against the truth on one call: the reach and the bins; and against the compiled merge for every n.  Returns the truth's reach."""
    A, N, P, hit = call
    want = HT.reach(N, P, A, hit, hist, cap) if motion is None else HT.reach_motion(N, P, A, hit, hist, motion[0], motion[1], motion[2], cap)
    for n in n_values:
        got, merged, got_bins = run_driver(driver, call, hist, cap, n, motion)
        assert same(got, want), "%d words of the reach differ from the truth" % int((bits(got) != bits(want)).sum())
        assert np.array_equal(got_bins, HT.bins(want, hit))
        assert int(got_bins.sum()) == int(np.asarray(hit).astype(bool).sum())  # the bins of a block sum to its hit pixels
        with np.errstate(all="ignore"):
            assert same(merged, np.where(want > 0, F(n) + want, F(n)).astype(np.float32)), "the merge's out.n is not n + reach (n = %r)" % n
    return want


def test_header_needs_no_hip_include_and_has_no_fma_exp_or_pow():
    text = open(os.path.join(DEVICE, "history_reach.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in "".join(l for l in code.splitlines() if l.startswith("#include")).lower()
    assert not re.search(r"\b(fmaf?|expf?|exp2f?|powf?|__builtin\w*)\b", code)
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", DEVICE, "-x", "c++", "-"],
                   input=b'#include "history_reach.hpp"\nint main() { return adypt::reach_bin(63.999f) == 63 && adypt::reach_bin(64.0f) == 64 ? 0 : 1; }\n', check=True)


# ---- hand-made histories ----
# The previous camera: at O, looking along R (0, 0, -1) with R a rotation of 0.5 rad about y, tan(fov / 2) = (0.75, 0.5).  The history shows a plane at
# depth 5 in front of it, every history pixel at its own pixel centre on the plane; the current call's pixels lie on the same plane wherever the case
# wants them to reproject.
O_PREV, TAN, DEPTH = np.array([0.25, -0.5, 1.0], np.float32), (0.75, 0.5), 5.0


def previous_camera():
    c, s = np.cos(0.5), np.sin(0.5)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], np.float64)  # columns: the camera's axes in the world
    inv_view = np.zeros(16, np.float32)
    for k in range(3):
        inv_view[4 * k:4 * k + 3] = R[:, k]
    inv_view[15] = 1.0
    inv_proj = np.zeros(16, np.float32)
    inv_proj[0], inv_proj[5], inv_proj[14] = TAN[0], TAN[1], -1.0  # a = (tx, 0, 0), b = (0, ty, 0), c = column 2 + column 3 = (0, 0, -1)
    return R, inv_proj, inv_view


def plane_point(R, w, h, fx, fy, depth=DEPTH):
    """The world point on the plane at `depth` that the previous camera sees at the continuous pixel coordinates (fx, fy) (binary64, then rounded)."""
    sx, sy = (np.asarray(fx, np.float64) + 0.5) * 2.0 / w - 1.0, 1.0 - (np.asarray(fy, np.float64) + 0.5) * 2.0 / h
    t = np.stack([sx * TAN[0] * depth, sy * TAN[1] * depth, -depth * np.ones_like(sx)], -1)
    return (O_PREV.astype(np.float64) + t @ R.T).astype(np.float32)


def at_edge(cam, R, w, h, edge, other, axis):
    """Two points on the plane whose reprojected fx (axis 0) or fy (axis 1) lies as near to `edge` as the arithmetic comes: the greatest value below
    it and the least one at or above it among 40 000 points a ten-millionth of a pixel apart (the edge itself where a point reaches it)."""
    a = np.float64(edge) + np.arange(-20000, 20000) * 1.0e-7
    o = np.full_like(a, other)
    p = plane_point(R, w, h, a if axis == 0 else o, o if axis == 0 else a)
    ok, gx, gy, _ = TT.reproject(cam, w, h, p[None])
    g = (gx if axis == 0 else gy)[0]
    assert ok.all()
    below, above = np.where(g < F(edge), g, -np.inf), np.where(g >= F(edge), g, np.inf)
    assert np.isfinite(below.max()) and np.isfinite(above.min()) and above.min() - below.max() < 1e-5
    return p[np.argmax(below)], p[np.argmin(above)]


def handmade(w, h, seed):
    """(call, hist, notes): a history in which every edge case of the issue occurs at a known pixel."""
    rng = np.random.RandomState(seed)
    R, inv_proj, inv_view = previous_camera()
    normal = R[:, 2].astype(np.float32)
    qy, qx = np.mgrid[0:h, 0:w]
    hP = plane_point(R, w, h, qx, qy)
    hN = np.broadcast_to(normal, (h, w, 3)).copy()
    hA = np.full((h, w, 3), 0.5, np.float32)
    hD = rng.rand(h, w, 3).astype(np.float32)
    hV = rng.rand(h, w).astype(np.float32)
    hn = rng.choice(np.array([1.0, 3.5, 17.0, 63.999, 64.0, 90.0], np.float32), size=(h, w)).astype(np.float32)  # lengths below, at and above the cap
    hhit = np.ones((h, w), bool)
    hist = TT.commit(hD, hV, hn, hN, hP, hA, hhit, O_PREV, inv_proj, inv_view)
    hist["raw_cam"] = np.concatenate([O_PREV, inv_proj, inv_view]).astype(np.float32)
    cam = hist["cam"]
    # where every current pixel reprojects to: its own place moved by a fraction of a pixel, then the edge cases at pixels of their own
    fx = qx + rng.uniform(-1.4, 1.4, (h, w))
    fy = qy + rng.uniform(-1.4, 1.4, (h, w))
    P = plane_point(R, w, h, fx, fy)
    N = np.broadcast_to(normal, (h, w, 3)).copy()
    A = np.full((h, w, 3), 0.5, np.float32)
    hit = np.ones((h, w), bool)
    # the edges of the image: fx == -1 and fx == width exactly, just inside them, and the same for fy; taps outside the image on every side
    P[0, 1], P[0, 0] = at_edge(cam, R, w, h, -1.0, 1.25, 0)       # fx < -1: refused; fx >= -1: its one column inside weighs (almost) nothing
    P[0, 2] = plane_point(R, w, h, -0.75, 2.5)
    P[0, 3] = plane_point(R, w, h, w - 0.25, 0.25)
    P[0, 4], P[0, 5] = at_edge(cam, R, w, h, float(w), 1.25, 0)   # fx < width; fx >= width: refused
    P[2, 5], P[2, 4] = at_edge(cam, R, w, h, -1.0, 2.5, 1)
    P[3, 4], P[3, 5] = at_edge(cam, R, w, h, float(h), 2.5, 1)
    P[0, 6] = plane_point(R, w, h, 3.5, -0.5)
    P[1, 0] = plane_point(R, w, h, 2.5, h - 0.5)
    P[1, 1] = plane_point(R, w, h, -3.0, 2.0)            # outside altogether
    P[1, 2] = plane_point(R, w, h, 2.25, 2.25, -DEPTH)   # behind the previous camera
    P[1, 3] = np.array([np.nan, 0.0, 0.0], np.float32)   # a NaN in the point
    hit[1, 4] = False                                    # a miss
    N[1, 5] = -normal                                    # another side of the surface
    A[1, 6] = (0.5, 0.5, 0.75)                           # another material
    # one tap of the four alone counts, its weight on either side of 0.01: history pixel (3, 3), whose three neighbours in the 2 x 2 are misses
    for k, u in enumerate((0.91, 0.9, 0.89, 0.85)):
        P[2, k] = plane_point(R, w, h, 3.0 + u, 3.0 + u)
    hist["hit"][3, 4] = hist["hit"][4, 3] = hist["hit"][4, 4] = False
    # lengths: 64 everywhere around history pixel (1, 1) — w * 64 is exact, so the reach is 64 to the bit — and 63.999 around (4, 1); n_q <= 0
    hist["n"][0:3, 0:3], hist["n"][0:3, 3:6] = 64.0, 63.999
    hist["n"][4, 0], hist["n"][4, 1] = 0.0, -3.0
    for k, (x, y) in enumerate(((1, 1), (4, 1), (0, 4), (1, 4))):
        P[3, k] = plane_point(R, w, h, float(x), float(y))
    # a NaN or an infinity in each of h0, h1, h2, ha and in n_q, at history pixels the pixels of row 4 reproject onto (the other taps then weigh nothing)
    hist["D"][2, 5, 1], hist["V"][2, 6], hist["N"][3, 5, 0], hist["P"][3, 6, 2], hist["A"][1, 5, 2] = np.nan, np.inf, np.nan, -np.inf, np.nan
    hist["n"][1, 6] = np.inf
    for k, (x, y) in enumerate(((5, 2), (6, 2), (5, 3), (6, 3), (5, 1), (6, 1), (5.5, 2.5))):
        P[4, k] = plane_point(R, w, h, float(x), float(y))
    return (A, N, P, hit), hist


@pytest.mark.parametrize("w,h", [(7, 5), (37, 33)])
def test_reach_is_the_truths_and_the_merges_on_handmade_histories(driver, w, h):
    call, hist = handmade(w, h, 5)
    reach = check(driver, call, hist)
    A, N, P, hit = call
    # the cases are what they are meant to be (by the truth): refused at the edges and behind the camera, found just inside; the lengths
    assert not reach[0, [0, 1, 4, 5]].any() and not reach[2, 4:6].any() and not reach[3, 4:6].any(), "at the edges -1 and width / height, from either side"
    assert reach[0, 2] > 0 and reach[0, 3] > 0 and reach[0, 6] > 0 and reach[1, 0] > 0, "two taps outside the image, two inside"
    assert not reach[1, 1:7].any(), "outside, behind the camera, a NaN, a miss, another normal, another albedo"
    assert reach[2, 0] == 0 and reach[2, 2] > 0 and reach[2, 3] > 0, "the sum of the weights on either side of 0.01"
    assert reach[3, 0] == F(64.0) and F(63.99) < reach[3, 1] < F(64.0) and reach[3, 2] == 0 and reach[3, 3] == 0
    assert HT.reach_bin(reach[3, 0]) == 64 and HT.reach_bin(reach[3, 1]) == 63 and HT.reach_bin(F(63.999)) == 63
    assert not reach[4, :7].any(), "a NaN or an infinity in h0, h1, h2, ha or n_q refuses the tap"
    assert np.isfinite(reach).all() and (reach >= 0).all() and (reach <= F(64.0)).all()
    # a cap below and above the lengths; no history at all
    low = check(driver, call, hist, cap=2.5, n_values=(3.0,))
    assert low.max() == F(2.5)
    high = check(driver, call, hist, cap=1000.0, n_values=(3.0,))
    assert high.max() == F(90.0) and same(np.minimum(high, F(64.0)), reach)
    none = check(driver, call, None, n_values=(3.0,))
    assert not none.any()


def test_the_motion_form_is_the_truths_and_the_motion_merges(driver):
    w, h = 37, 33
    call, hist = handmade(w, h, 9)
    A, N, P, hit = call
    rng = np.random.RandomState(2)
    n_tris = 6
    prev = TM.tri_words(rng.uniform(-1, 1, (n_tris, 3, 3)), rng.uniform(-1, 1, (n_tris, 3, 3)))
    cur = prev.copy()
    cur[1, :9] += F(0.05)          # a triangle that moved a little
    cur[2, :] = -cur[2, :]         # one that turned over
    prev[3, 9:18] = 0.0            # one whose previous normals give no direction: not valid, no history
    cur[3, 0] += F(1.0)
    hist["tris"] = prev[:5].copy()  # triangle 5 is a stranger to the snapshot
    tri = rng.randint(-1, n_tris, (h, w)).astype(np.int32)
    uv = rng.uniform(0.0, 0.5, (h, w, 2)).astype(np.float32)
    hit = hit & (tri != -1)
    reach = check(driver, (A, N, P, hit), hist, motion=(tri, uv, cur))
    still = HT.reach(N, P, A, hit, hist)
    unmoved = np.isin(tri, (0, 4, 5))
    assert same(reach[unmoved], still[unmoved]), "an unmoved triangle and a stranger reach as the still form does"
    assert not reach[(tri == 3) & hit].any()
    hist["tris"] = None
    assert same(check(driver, (A, N, P, hit), hist, motion=(tri, uv, cur), n_values=(2.0,)), still), "no snapshot: the still form"
