// Variance from temporal luminance moments: what lets a temporal call run from 1 spp per pose.  denoise_prepare needs n >= 2 for V0 = m2 / (n (n - 1)).
// A moments call carries, in the fourth channel of the merged image and of the history, the per-sample raw second moment S of the demodulated luminance
// instead of a variance; S is blended over the history like a colour, and the variance the levels see is made per pixel AFTER the merge:
//     own = max(S - lum(D)^2, 0)
//     a miss pixel, and a hit pixel whose history is at least kMomentsMinLength samples long:   V = own / n_out
//     a hit pixel with a shorter history: over the (2 kMomentsRadius + 1)^2 window of the merged image, the taps on the pixel's surface (rectify_tap's
//     tests against the centre, under the CURRENT camera) give mu1 = sum lum(D_q) / k, mu2 = sum S_q / k, sigma2 = max(mu2 - mu1^2, 0), and
//     V = sigma2 / n_out where k >= kMomentsMinTaps, own / n_out otherwise
// (SVGF's two parts: temporal moments, and a spatial estimate while the history is short).  No first moment is stored: lum(D) of the merged colour is it.
// THE definition for host and device (no HIP needed).  temporal.hpp includes it beside rectify.hpp, whose centre and constants it uses: include
// temporal.hpp, not this.  Canonical arithmetic as there: binary32, the operations in the order written, NO fma, only + - * / sqrtf fabsf, comparisons
// and selects, every refusal written so that a NaN refuses; tests/moments_truth.py restates it in numpy float32 bit for bit.  The merge of a moments
// call is temporal_merge_through<true> (temporal.hpp): its taps, tests, weights, cap and colour blend, the fourth channel blended with w, not w^2.
#pragma once

namespace adypt {

constexpr int kMomentsMinLength = 4; // the constants are part of the definition, not tunables
constexpr int kMomentsRadius = 3;
constexpr int kMomentsMinTaps = 4;

// level 0 of a moments call: (D0.rgb, S0), S0 = Y^2 + (m2 / n) / la^2 — defined for n >= 1, Y^2 at n = 1 (m2 = 0)
ADYPT_HOST_DEVICE Dn4 moments_prepare(float cr, float cg, float cb, float m2, float n, float ar, float ag, float ab)
{
	const float la = noise_luminance(ar, ag, ab) + kDenoiseAlbedoFloor;
	Dn4 r;
	r.x = cr / (ar + kDenoiseAlbedoFloor); r.y = cg / (ag + kDenoiseAlbedoFloor); r.z = cb / (ab + kDenoiseAlbedoFloor);
	const float y = noise_luminance(r.x, r.y, r.z);
	r.w = y * y + (m2 / n) / (la * la);
	return r;
}

// own = max(S - Y^2, 0) (a NaN becomes 0)
ADYPT_HOST_DEVICE float moments_own(float y, float s)
{
	const float own = s - y * y;
	return own > 0.0f ? own : 0.0f;
}

// whether a pixel asks its window: a hit whose merged history is shorter than kMomentsMinLength (a NaN length does not ask)
ADYPT_HOST_DEVICE bool moments_wants_window(bool hit, float n_out) { return hit && n_out < (float)kMomentsMinLength; }

struct MomentsSums { float k, s1, s2; };

// One tap inside the image against the centre `c` (rectify_centre of the merged call's guides): rectify_tap's tests — hit, normal, plane, albedo — and
// finite lum(D_q) = qy and S_q = qs.  A tap that does not count is skipped whole.
ADYPT_HOST_DEVICE void moments_tap(const RectifyCentre &c, MomentsSums &s, float qnx, float qny, float qnz, float qhit, float qpx, float qpy, float qpz, float qar, float qag, float qab,
                                   float qy, float qs)
{
	if(!(qhit != 0.0f)) return;
	if(!((c.nx * qnx + c.ny * qny) + c.nz * qnz >= kTemporalNormalMin)) return;
	const float dx = qpx - c.px, dy = qpy - c.py, dz = qpz - c.pz;
	if(!(fabsf((c.nx * dx + c.ny * dy) + c.nz * dz) <= c.tol)) return;
	if(!(fabsf(qar - c.ar) <= kTemporalAlbedoTol && fabsf(qag - c.ag) <= kTemporalAlbedoTol && fabsf(qab - c.ab) <= kTemporalAlbedoTol)) return;
	if(!(fabsf(qy) <= kTemporalFiniteMax && fabsf(qs) <= kTemporalFiniteMax)) return;
	s.k = s.k + 1.0f;
	s.s1 = s.s1 + qy;
	s.s2 = s.s2 + qs;
}

struct MomentsVariance { float v; bool spatial; }; // spatial: the pixel took the window estimate

// own, n_out of the pixel; `windowed`: the pixel asked its window (moments_wants_window) and s are its sums
ADYPT_HOST_DEVICE MomentsVariance moments_finish(float own, float n_out, bool windowed, const MomentsSums &s)
{
	MomentsVariance r{own / n_out, false};
	if(!windowed || !(s.k >= (float)kMomentsMinTaps)) return r;
	const float mu1 = s.s1 / s.k, mu2 = s.s2 / s.k;
	float var = mu2 - mu1 * mu1;
	var = var > 0.0f ? var : 0.0f;
	r.v = var / n_out;
	r.spatial = true;
	return r;
}

// The variance at pixel (px, py) of the merged images: `img` answers x0(i) = (D.rgb, S), x1(i) = (N.xyz, hit), x2(i) = (P.xyz, n_out), xa(i) for the
// row-major pixel index i; o is the current camera's origin.  The taps are visited row by row, dy outside and dx inside, the centre included: the order
// of the sums is part of the definition.
template <class Img> ADYPT_HOST_DEVICE MomentsVariance moments_variance(const Img &img, int width, int height, int px, int py, const float *o)
{
	const int p = py * width + px;
	const Dn4 c0 = img.x0(p), c1 = img.x1(p), c2 = img.x2(p);
	const float own = moments_own(noise_luminance(c0.x, c0.y, c0.z), c0.w);
	MomentsSums s{0.0f, 0.0f, 0.0f};
	const bool windowed = moments_wants_window(c1.w != 0.0f, c2.w);
	if(!windowed) return moments_finish(own, c2.w, false, s);
	const RectifyCentre c = rectify_centre(c1, c2, img.xa(p), o);
	for(int dy = -kMomentsRadius; dy <= kMomentsRadius; ++dy)
		for(int dx = -kMomentsRadius; dx <= kMomentsRadius; ++dx)
		{
			const int qx = px + dx, qy = py + dy;
			if(qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
			const int q = qy * width + qx;
			const Dn4 q1 = img.x1(q), q2 = img.x2(q), qa = img.xa(q), q0 = img.x0(q);
			moments_tap(c, s, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, qa.x, qa.y, qa.z, noise_luminance(q0.x, q0.y, q0.z), q0.w);
		}
	return moments_finish(own, c2.w, true, s);
}

}  // namespace adypt
