// The temporal half of SVGF: what the last committing call left (the history) is reprojected through the primary hit of the current call and counted
// as further samples where the surface is still the same; the a-trous levels of denoise.hpp then run unchanged on the merged (D, V).
// THE definition for host and device (no HIP needed: tests/test_temporal_definition.py compiles it on the host with -ffp-contract=off).  Canonical
// arithmetic as in denoise.hpp: binary32, round to nearest, the operations in the order written, NO fma, no exp / pow — only + - * / sqrtf floorf
// fabsf, comparisons and selects — so that the numpy float32 restatement (tests/temporal_truth.py) is bit-exact.  Every comparison is written so that
// a NaN yields "no history", and every float is range-tested before it is converted to int.  (Following moved geometry, at the end, also compares words
// as bits: tests/temporal_motion_truth.py restates that part.)
//
// The history, row-major float4 images at the picture's coordinates of the call that committed it, and that call's camera:
//     H0 = (D.rgb, V)   the merged PRE-filter state (not the filtered result: no blur accumulates over calls)
//     H1 = (N.xyz, hit) H2 = (P.xyz, n_out)  HA = (A.rgb, .)
// 64 B per pixel; the merged image of the current call (16 B) and the history length read-out (4 B) beside it: 84 B per pixel in all, allocated at
// the first temporal call.  A commit swaps buffers with the current call's images, nothing is copied.
#pragma once
#include "denoise.hpp"
#include <cstdint>
#include <cstring>

namespace adypt {

constexpr float kTemporalNormalMin = 0.9f;   // N . N_q of a tap that counts; the constants are part of the definition, not tunables
constexpr float kTemporalPlaneTol = 0.02f;   // |N . (P_q - P)| as a fraction of the distance of P from the previous camera
constexpr float kTemporalAlbedoTol = 0.1f;   // max |A_q - A|: demodulated history of another material is not multiplied by this one's albedo
constexpr float kTemporalMinWeight = 0.01f;  // the bilinear weight the counting taps have to bring together
constexpr float kTemporalFiniteMax = 3.0e38f; // a history tap holding a value beyond it (an infinity, a NaN) does not count
constexpr float kTemporalDefaultCap = 64.0f;

// (written so that a NaN, an infinity and anything not positive are refused)
inline bool temporal_cap_valid(float cap) { return cap > 0.0f && cap <= kTemporalFiniteMax; }

}  // namespace adypt

#include "rectify.hpp" // rectifying stale history against the current call's own neighbourhood: the window statistics and the clamp (uses the constants above)
#include "moments.hpp" // a moments call (from 1 spp per pose): the fourth channel is a raw second moment S, the variance is made after the merge (uses both)

namespace adypt {

// The camera of the call that left the history, made only of what adypt_set_camera was given: the screen point (sx, sy) has the camera-space
// direction t = a sx + b sy + c (columns 0, 1 and 2 + 3 of inv_proj, as camera_dir in shade.hpp), the world direction is R t with R the upper 3 x 3
// of inv_view, kept here as its columns r[0..2], r[3..5], r[6..8].
struct TemporalCamera { float o[3], a[3], b[3], c[3], r[9]; };

ADYPT_HOST_DEVICE TemporalCamera temporal_camera(const float *origin, const float *inv_proj, const float *inv_view)
{
	TemporalCamera cam;
	for(int i = 0; i < 3; ++i)
	{
		cam.o[i] = origin[i];
		cam.a[i] = inv_proj[i]; cam.b[i] = inv_proj[4 + i]; cam.c[i] = inv_proj[8 + i] + inv_proj[12 + i];
		cam.r[i] = inv_view[i]; cam.r[3 + i] = inv_view[4 + i]; cam.r[6 + i] = inv_view[8 + i];
	}
	return cam;
}

// The continuous pixel coordinates (*fx, *fy) at which the previous camera saw the world point p, and the distance of p from that camera; false
// when it saw it nowhere (behind it, a singular system, a NaN anywhere).  No 4 x 4 inverse: t || v is solved for (sx, sy) by Cramer's rule on the
// x / z and y / z components, v = R^T (p - o).
ADYPT_HOST_DEVICE bool temporal_reproject(const TemporalCamera &cam, int width, int height, float px, float py, float pz, float *fx, float *fy, float *dist)
{
	const float ex = px - cam.o[0], ey = py - cam.o[1], ez = pz - cam.o[2];
	*dist = sqrtf((ex * ex + ey * ey) + ez * ez);
	const float vx = (cam.r[0] * ex + cam.r[1] * ey) + cam.r[2] * ez;
	const float vy = (cam.r[3] * ex + cam.r[4] * ey) + cam.r[5] * ez;
	const float vz = (cam.r[6] * ex + cam.r[7] * ey) + cam.r[8] * ez;
	const float m00 = cam.a[0] * vz - cam.a[2] * vx, m01 = cam.b[0] * vz - cam.b[2] * vx, r0 = cam.c[2] * vx - cam.c[0] * vz;
	const float m10 = cam.a[1] * vz - cam.a[2] * vy, m11 = cam.b[1] * vz - cam.b[2] * vy, r1 = cam.c[2] * vy - cam.c[1] * vz;
	const float det = m00 * m11 - m01 * m10;
	if(!(fabsf(det) > 0.0f)) return false;
	const float sx = (r0 * m11 - m01 * r1) / det, sy = (m00 * r1 - r0 * m10) / det;
	const float tx = (cam.a[0] * sx + cam.b[0] * sy) + cam.c[0];
	const float ty = (cam.a[1] * sx + cam.b[1] * sy) + cam.c[1];
	const float tz = (cam.a[2] * sx + cam.b[2] * sy) + cam.c[2];
	if(!((tx * vx + ty * vy) + tz * vz > 0.0f)) return false; // behind the camera
	*fx = ((sx + 1.0f) * (float)width) * 0.5f - 0.5f;
	*fy = ((1.0f - sy) * (float)height) * 0.5f - 0.5f; // (camera_dir negates sy)
	return true;
}

// What the merge leaves at a pixel: the merged (D.rgb, V) and the effective sample count n_out; of a rectified merge also the share of its length the
// history kept (1 where the pixel found no history, or was not rectified).
struct TemporalOut { Dn4 x0; float n; float kept; };

// The body of both forms of the merge: the pixel's surface as the HISTORY holds it — its normal (nx, ny, nz) and its point (px, py, pz) at the time of the
// last commit — is what is reprojected and what a tap's normal and plane are held against.  temporal_merge gives the current normal and point (the
// surface stands still), temporal_merge_motion what temporal_previous_point made of the hit triangle as it was then.
// rect.on (rectify.hpp): where the window of the pixel has at least kRectifyMinTaps taps, the history's colour is clamped to the window's mean within
// gamma * sqrt(g) per channel and its length multiplied by f before the blend; a length that is then not positive takes no history.  hv stays.
// MOMENTS (moments.hpp): the fourth channel of c0 and of the history is the raw second moment S, blended like a colour — S_h = sum w S_q / sum w,
// S = (n S0 + n_h S_h) / (n + n_h); a compile-time constant, so that the other instances are what they were.
// VIRTUAL (temporal_merge_virtual, below): the point reprojected through the history's camera, and whose distance from it scales the plane tolerance, is
// (vx, vy, vz) — the pixel's virtual point — while a tap's normal and plane are still held against (n, p), which are then the FOLLOWED guides; and a tap
// counts only where its class is `cls`, the centre's.  A compile-time constant too: the other instances never look at the last four arguments.
template <bool MOMENTS = false, bool VIRTUAL = false, class Hist>
ADYPT_HOST_DEVICE TemporalOut temporal_merge_through(const Hist &hist, bool have, const TemporalCamera &cam, int width, int height, const Dn4 &c0, bool hit, float nx, float ny, float nz,
                                                     float px, float py, float pz, const Dn4 &ca, float n, float history_cap, const Rectify rect = Rectify{}, float cls = 0.0f,
                                                     float vx = 0.0f, float vy = 0.0f, float vz = 0.0f)
{
	TemporalOut out;
	out.x0 = c0; out.n = n; out.kept = 1.0f;
	if(!have || !hit) return out;
	float fx, fy, dist;
	if(!temporal_reproject(cam, width, height, VIRTUAL ? vx : px, VIRTUAL ? vy : py, VIRTUAL ? vz : pz, &fx, &fy, &dist)) return out;
	// floorf(fx) in [-1, width - 1]: one of the two columns at least lies inside (and a NaN is refused)
	if(!(fx >= -1.0f && fx < (float)width && fy >= -1.0f && fy < (float)height)) return out;
	const float bx = floorf(fx), by = floorf(fy);
	const int ix = (int)bx, iy = (int)by;
	const float ux = fx - bx, uy = fy - by;
	const float tol = kTemporalPlaneTol * dist;
	float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, sn = 0.0f;
	for(int ty = 0; ty <= 1; ++ty)
		for(int tx = 0; tx <= 1; ++tx)
		{
			const int qx = ix + tx, qy = iy + ty;
			if(qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
			const int q = qy * width + qx;
			const Dn4 q1 = hist.h1(q);
			if(VIRTUAL ? !(q1.w == cls) : !(q1.w != 0.0f)) continue;
			if(!((nx * q1.x + ny * q1.y) + nz * q1.z >= kTemporalNormalMin)) continue;
			const Dn4 q2 = hist.h2(q);
			const float dx = q2.x - px, dy = q2.y - py, dz = q2.z - pz;
			if(!(fabsf((nx * dx + ny * dy) + nz * dz) <= tol)) continue;
			const Dn4 qa = hist.ha(q);
			if(!(fabsf(qa.x - ca.x) <= kTemporalAlbedoTol && fabsf(qa.y - ca.y) <= kTemporalAlbedoTol && fabsf(qa.z - ca.z) <= kTemporalAlbedoTol)) continue;
			const Dn4 q0 = hist.h0(q);
			if(!(fabsf(q0.x) <= kTemporalFiniteMax && fabsf(q0.y) <= kTemporalFiniteMax && fabsf(q0.z) <= kTemporalFiniteMax && fabsf(q0.w) <= kTemporalFiniteMax &&
			     q2.w > 0.0f && q2.w <= kTemporalFiniteMax)) continue;
			const float w = (tx == 0 ? 1.0f - ux : ux) * (ty == 0 ? 1.0f - uy : uy);
			sw = sw + w;
			sr = sr + w * q0.x; sg = sg + w * q0.y; sb = sb + w * q0.z;
			sv = sv + (MOMENTS ? w : w * w) * q0.w;
			sn = sn + w * q2.w;
		}
	if(!(sw > kTemporalMinWeight)) return out;
	float hr = sr / sw, hg = sg / sw, hb = sb / sw;
	const float hv = MOMENTS ? sv / sw : sv / (sw * sw);
	const float hq = sn / sw;
	float nh = hq < history_cap ? hq : history_cap;
	if(rect.on && rect.r0.w >= (float)kRectifyMinTaps)
	{
		out.kept = rectify_history(rect, &hr, &hg, &hb);
		nh = nh * out.kept;
		if(!(nh > 0.0f)) return out;
	}
	const float den = n + nh;
	out.x0.x = (n * c0.x + nh * hr) / den; out.x0.y = (n * c0.y + nh * hg) / den; out.x0.z = (n * c0.z + nh * hb) / den;
	out.x0.w = MOMENTS ? (n * c0.w + nh * hv) / den : ((n * n) * c0.w + (nh * nh) * hv) / (den * den);
	out.n = den;
	return out;
}

// The merge at pixel (px, py).  c0 = (D0.rgb, V0) of denoise_prepare, c1 = (N.xyz, hit), c2 = (P.xyz, .), ca = (A.rgb, .) of the current call, n the
// sample count of the pixel's block.  `hist` answers h0(i), h1(i), h2(i), ha(i) for the row-major pixel index i of the history; have = false: there
// is none.  A tap that does not count is skipped entirely (an accumulator keeps its word).
template <bool MOMENTS = false, class Hist>
ADYPT_HOST_DEVICE TemporalOut temporal_merge(const Hist &hist, bool have, const TemporalCamera &cam, int width, int height, const Dn4 &c0, const Dn4 &c1, const Dn4 &c2, const Dn4 &ca,
                                             float n, float history_cap, const Rectify rect = Rectify{})
{
	return temporal_merge_through<MOMENTS>(hist, have, cam, width, height, c0, c1.w != 0.0f, c1.x, c1.y, c1.z, c2.x, c2.y, c2.z, ca, n, history_cap, rect);
}

// ---- through mirrors and glass: the merge by the virtual point (adypt_denoise_temporal_specular) ----
// The call's guides are the FOLLOWED ones of guide_chain.hpp: c1 = (N.xyz, class), c2 = (P.xyz, .), ca = (A.rgb, .) of the surface the pixel's chain
// ended on, and xv = (Pv.xyz, len): the virtual point of a followed pixel (class >= 2) and the unfolded length it was made with, 0 where that length is
// not valid (chain_virtual_point); of every other pixel xv is (P, 0) and is not looked at.  Who takes no history: a pixel with !(class >= 1) — a primary
// miss, an escaped chain, a NaN — and a followed pixel whose virtual point is not valid.  A class 1 pixel is its own virtual point.  The point
// reprojected is Pv and dist = |Pv - O_prev|; a tap counts where it lies inside the image, its class EQUALS the centre's, N . N_q >= 0.9,
// |N . (P_q - P)| <= 0.02 dist, max |A_q - A| <= 0.1 — all on the followed guides — and its values are finite with n_q > 0; the weights, the least
// weight, the cap, the blend and n_out are temporal_merge's.  For class 1 this is temporal_merge with the stricter class test: on a history whose
// classes are all 0 or 1 the same bits.  No rectified, moments or motion form.
template <class Hist>
ADYPT_HOST_DEVICE TemporalOut temporal_merge_virtual(const Hist &hist, bool have, const TemporalCamera &cam, int width, int height, const Dn4 &c0, const Dn4 c1, const Dn4 c2, const Dn4 &ca,
                                                     const Dn4 xv, float n, float history_cap)
{
	const float cls = c1.w;
	const bool followed = cls >= 2.0f;
	const bool takes = cls >= 1.0f && (!followed || (xv.w > 0.0f && xv.w <= kTemporalFiniteMax));
	float vx = c2.x, vy = c2.y, vz = c2.z;
	if(followed) { vx = xv.x; vy = xv.y; vz = xv.z; }
	return temporal_merge_through<false, true>(hist, have, cam, width, height, c0, takes, c1.x, c1.y, c1.z, c2.x, c2.y, c2.z, ca, n, history_cap, Rectify{}, cls, vx, vy, vz);
}

// ---- following moved geometry ----
// The other half of SVGF's reprojection.  A committing motion call keeps words 0..17 of every triangle record (p0 p1 p2 n0 n1 n2) beside the history;
// a later call asks where the point it hit on a triangle WAS then, and merges through that point and that normal.  A triangle keeps its index across
// adypt_update_triangles, adypt_pose and adypt_rebuild_bvh, which is all the correspondence there is.
constexpr int kTemporalTriWords = 18;

// where the pixel's surface was when the history was committed: xp = (P_prev.xyz, moved ? 1 : 0), xn = (N_prev.xyz, valid ? 1 : 0)
struct TemporalPrevious { Dn4 xp, xn; };

ADYPT_HOST_DEVICE bool temporal_same_word(float a, float b)
{
	uint32_t x, y;
	memcpy(&x, &a, 4); memcpy(&y, &b, 4);
	return x == y;
}

// prev, cur: words 0..17 of the hit triangle's record then and now, looked at only when `known` — the pixel hit a triangle whose index lies inside the
// snapshot; (u, v) of the hit; c1, c2 of the current call.  Unmoved (not known: sky, a stranger; or all 18 words equal as bits): the current normal and
// point, so that the merge is temporal_merge to the bit.  Moved: the hit's barycentric combination of the previous vertices, weighted as viewer_color
// weighs them (p0 by u, p1 by v, p2 by w), and of the previous normals, normalised; not valid — no history — when the squared length of that normal
// is not a positive finite number.
ADYPT_HOST_DEVICE TemporalPrevious temporal_previous_point(const float *prev, const float *cur, bool known, float u, float v, const Dn4 &c1, const Dn4 &c2)
{
	TemporalPrevious r;
	r.xp = Dn4{c2.x, c2.y, c2.z, 0.0f};
	r.xn = Dn4{c1.x, c1.y, c1.z, 1.0f};
	if(!known) return r;
	bool same = true;
	for(int k = 0; k < kTemporalTriWords; ++k) same = same && temporal_same_word(prev[k], cur[k]);
	if(same) return r;
	const float w = (1.0f - u) - v;
	const float px = (prev[0] * u + prev[3] * v) + prev[6] * w, py = (prev[1] * u + prev[4] * v) + prev[7] * w, pz = (prev[2] * u + prev[5] * v) + prev[8] * w;
	const float nx = (prev[9] * u + prev[12] * v) + prev[15] * w, ny = (prev[10] * u + prev[13] * v) + prev[16] * w, nz = (prev[11] * u + prev[14] * v) + prev[17] * w;
	const float len2 = (nx * nx + ny * ny) + nz * nz;
	r.xp = Dn4{px, py, pz, 1.0f};
	if(!(len2 > 0.0f && len2 <= kTemporalFiniteMax)) { r.xn = Dn4{0.0f, 0.0f, 0.0f, 0.0f}; return r; }
	const float len = sqrtf(len2);
	r.xn = Dn4{nx / len, ny / len, nz / len, 1.0f};
	return r;
}

// The motion form of the merge: through (P_prev, N_prev).  The call's own (D0, V0), and the X1 / X2 that become history on a commit, stay the current
// pose's; the albedo test, the finiteness tests, the weights, the cap and the blend are temporal_merge's.
template <bool MOMENTS = false, class Hist>
ADYPT_HOST_DEVICE TemporalOut temporal_merge_motion(const Hist &hist, bool have, const TemporalCamera &cam, int width, int height, const Dn4 &c0, const Dn4 &c1, const Dn4 &ca, float n,
                                                    float history_cap, const Dn4 &xp, const Dn4 &xn, const Rectify rect = Rectify{})
{
	return temporal_merge_through<MOMENTS>(hist, have && xn.w != 0.0f, cam, width, height, c0, c1.w != 0.0f, xn.x, xn.y, xn.z, xp.x, xp.y, xp.z, ca, n, history_cap, rect);
}

}  // namespace adypt
