// The temporal half of SVGF: what the last committing call left (the history) is reprojected through the primary hit of the current call and counted
// as further samples where the surface is still the same; the a-trous levels of denoise.hpp then run unchanged on the merged (D, V).
// THE definition for host and device (no HIP needed: tests/test_temporal_definition.py compiles it on the host with -ffp-contract=off).  Canonical
// arithmetic as in denoise.hpp: binary32, round to nearest, the operations in the order written, NO fma, no exp / pow — only + - * / sqrtf floorf
// fabsf, comparisons and selects — so that the numpy float32 restatement (tests/temporal_truth.py) is bit-exact.  Every comparison is written so that
// a NaN yields "no history", and every float is range-tested before it is converted to int.
//
// The history, row-major float4 images at the picture's coordinates of the call that committed it, and that call's camera:
//     H0 = (D.rgb, V)   the merged PRE-filter state (not the filtered result: no blur accumulates over calls)
//     H1 = (N.xyz, hit) H2 = (P.xyz, n_out)  HA = (A.rgb, .)
// 64 B per pixel; the merged image of the current call (16 B) and the history length read-out (4 B) beside it: 84 B per pixel in all, allocated at
// the first temporal call.  A commit swaps buffers with the current call's images, nothing is copied.
#pragma once
#include "denoise.hpp"

namespace adypt {

constexpr float kTemporalNormalMin = 0.9f;   // N . N_q of a tap that counts; the constants are part of the definition, not tunables
constexpr float kTemporalPlaneTol = 0.02f;   // |N . (P_q - P)| as a fraction of the distance of P from the previous camera
constexpr float kTemporalAlbedoTol = 0.1f;   // max |A_q - A|: demodulated history of another material is not multiplied by this one's albedo
constexpr float kTemporalMinWeight = 0.01f;  // the bilinear weight the counting taps have to bring together
constexpr float kTemporalFiniteMax = 3.0e38f; // a history tap holding a value beyond it (an infinity, a NaN) does not count
constexpr float kTemporalDefaultCap = 64.0f;

// (written so that a NaN, an infinity and anything not positive are refused)
inline bool temporal_cap_valid(float cap) { return cap > 0.0f && cap <= kTemporalFiniteMax; }

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

// What the merge leaves at a pixel: the merged (D.rgb, V) and the effective sample count n_out.
struct TemporalOut { Dn4 x0; float n; };

// The merge at pixel (px, py).  c0 = (D0.rgb, V0) of denoise_prepare, c1 = (N.xyz, hit), c2 = (P.xyz, .), ca = (A.rgb, .) of the current call, n the
// sample count of the pixel's block.  `hist` answers h0(i), h1(i), h2(i), ha(i) for the row-major pixel index i of the history; have = false: there
// is none.  A tap that does not count is skipped entirely (an accumulator keeps its word).
template <class Hist>
ADYPT_HOST_DEVICE TemporalOut temporal_merge(const Hist &hist, bool have, const TemporalCamera &cam, int width, int height, const Dn4 &c0, const Dn4 &c1, const Dn4 &c2, const Dn4 &ca,
                                             float n, float history_cap)
{
	TemporalOut out;
	out.x0 = c0; out.n = n;
	if(!have || !(c1.w != 0.0f)) return out;
	float fx, fy, dist;
	if(!temporal_reproject(cam, width, height, c2.x, c2.y, c2.z, &fx, &fy, &dist)) return out;
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
			if(!(q1.w != 0.0f)) continue;
			if(!((c1.x * q1.x + c1.y * q1.y) + c1.z * q1.z >= kTemporalNormalMin)) continue;
			const Dn4 q2 = hist.h2(q);
			const float dx = q2.x - c2.x, dy = q2.y - c2.y, dz = q2.z - c2.z;
			if(!(fabsf((c1.x * dx + c1.y * dy) + c1.z * dz) <= tol)) continue;
			const Dn4 qa = hist.ha(q);
			if(!(fabsf(qa.x - ca.x) <= kTemporalAlbedoTol && fabsf(qa.y - ca.y) <= kTemporalAlbedoTol && fabsf(qa.z - ca.z) <= kTemporalAlbedoTol)) continue;
			const Dn4 q0 = hist.h0(q);
			if(!(fabsf(q0.x) <= kTemporalFiniteMax && fabsf(q0.y) <= kTemporalFiniteMax && fabsf(q0.z) <= kTemporalFiniteMax && fabsf(q0.w) <= kTemporalFiniteMax &&
			     q2.w > 0.0f && q2.w <= kTemporalFiniteMax)) continue;
			const float w = (tx == 0 ? 1.0f - ux : ux) * (ty == 0 ? 1.0f - uy : uy);
			sw = sw + w;
			sr = sr + w * q0.x; sg = sg + w * q0.y; sb = sb + w * q0.z;
			sv = sv + (w * w) * q0.w;
			sn = sn + w * q2.w;
		}
	if(!(sw > kTemporalMinWeight)) return out;
	const float hr = sr / sw, hg = sg / sw, hb = sb / sw, hv = sv / (sw * sw);
	const float hq = sn / sw;
	const float nh = hq < history_cap ? hq : history_cap;
	const float den = n + nh;
	out.x0.x = (n * c0.x + nh * hr) / den; out.x0.y = (n * c0.y + nh * hg) / den; out.x0.z = (n * c0.z + nh * hb) / den;
	out.x0.w = ((n * n) * c0.w + (nh * nh) * hv) / (den * den);
	out.n = den;
	return out;
}

}  // namespace adypt
