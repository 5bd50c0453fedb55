// Rectifying stale history: the temporal merge (temporal.hpp) accepts a history tap on geometry alone, so where the surface stands still but its LIGHT
// changed — a door that opened, a shadow that wandered, another sun — up to history_cap stale samples outvote the pose's own few.  Here the history is
// held against what the current call's own neighbourhood says: the mean of a (2 r + 1)^2 window of taps on the pixel's surface, and how far a value of
// that surface may lie from it.  A history that disagrees by m times that limit is clamped to the limit and keeps 1 / m of its length.
// THE definition for host and device (no HIP needed).  temporal.hpp includes it below its constants, which it uses: include temporal.hpp, not this.
// Canonical arithmetic as there: binary32, the operations in the order written, NO fma, only + - * / sqrtf fabsf, comparisons and selects, every
// refusal written as !(comparison) so that a NaN refuses; tests/rectify_truth.py restates it in numpy float32 bit for bit.
//
// Two row-major float4 images of the current call, 32 B per pixel:  R0 = (mu.rgb, k)   the window's mean and its number of counting taps
//                                                                   R1 = (g.rgb, 0)    the squared limit at gamma = 1
#pragma once

namespace adypt {

constexpr int kRectifyMinTaps = 4;           // a window of fewer counting taps says nothing: the pixel's history stays as it is
constexpr int kRectifyDefaultRadius = 3;     // the constants are part of the definition, not tunables
constexpr int kRectifyMaxRadius = 3;
constexpr float kRectifyDefaultGamma = 1.0f;

// (written so that a NaN is refused)
inline bool rectify_params_valid(int radius, float gamma) { return radius >= 1 && radius <= kRectifyMaxRadius && gamma >= 0.0f && gamma <= kTemporalFiniteMax; }

struct RectifyStats { Dn4 r0, r1; };

// The centre of a window: what a tap is held against.  tol = kTemporalPlaneTol * the distance of P from the CURRENT camera's origin o.
struct RectifyCentre { float nx, ny, nz, px, py, pz, ar, ag, ab, tol; };

ADYPT_HOST_DEVICE RectifyCentre rectify_centre(const Dn4 &c1, const Dn4 &c2, const Dn4 &ca, const float *o)
{
	const float ex = c2.x - o[0], ey = c2.y - o[1], ez = c2.z - o[2];
	const float dist = sqrtf((ex * ex + ey * ey) + ez * ez);
	return RectifyCentre{c1.x, c1.y, c1.z, c2.x, c2.y, c2.z, ca.x, ca.y, ca.z, kTemporalPlaneTol * dist};
}

struct RectifySums { float k, sr, sg, sb, tr, tg, tb, v; };

// One tap inside the image: (nx, ny, nz, hit) of X1, the point of X2, the albedo, (D0.rgb, V0) of X0.  A tap that does not count is skipped whole.
ADYPT_HOST_DEVICE void rectify_tap(const RectifyCentre &c, RectifySums &s, float qnx, float qny, float qnz, float qhit, float qpx, float qpy, float qpz, float qar, float qag, float qab,
                                   float qr, float qg, float qb, float qv)
{
	if(!(qhit != 0.0f)) return;
	if(!((c.nx * qnx + c.ny * qny) + c.nz * qnz >= kTemporalNormalMin)) return;
	const float dx = qpx - c.px, dy = qpy - c.py, dz = qpz - c.pz;
	if(!(fabsf((c.nx * dx + c.ny * dy) + c.nz * dz) <= c.tol)) return;
	if(!(fabsf(qar - c.ar) <= kTemporalAlbedoTol && fabsf(qag - c.ag) <= kTemporalAlbedoTol && fabsf(qab - c.ab) <= kTemporalAlbedoTol)) return;
	if(!(fabsf(qr) <= kTemporalFiniteMax && fabsf(qg) <= kTemporalFiniteMax && fabsf(qb) <= kTemporalFiniteMax && fabsf(qv) <= kTemporalFiniteMax)) return;
	s.k = s.k + 1.0f;
	s.sr = s.sr + qr; s.sg = s.sg + qg; s.sb = s.sb + qb;
	s.tr = s.tr + qr * qr; s.tg = s.tg + qg * qg; s.tb = s.tb + qb * qb;
	s.v = s.v + qv;
}

// var = t / k - mu * mu floored at 0 (a NaN — sums that overflowed — becomes 0); g = the surface's spatial spread, the variance of the window less its
// own sampling noise vn (V0 is the variance of the pixel mean, in luminance, and serves every channel), plus the standard error of the window mean
ADYPT_HOST_DEVICE float rectify_limit2(float t, float mu, float k, float vn)
{
	float var = t / k - mu * mu;
	var = var > 0.0f ? var : 0.0f;
	float e = var - vn;
	e = e > 0.0f ? e : 0.0f;
	return e + var / k;
}

ADYPT_HOST_DEVICE RectifyStats rectify_finish(const RectifySums &s)
{
	RectifyStats r;
	r.r0 = Dn4{0.0f, 0.0f, 0.0f, s.k};
	r.r1 = Dn4{0.0f, 0.0f, 0.0f, 0.0f};
	if(!(s.k > 0.0f)) return r;
	r.r0.x = s.sr / s.k; r.r0.y = s.sg / s.k; r.r0.z = s.sb / s.k;
	const float vn = s.v / s.k;
	r.r1.x = rectify_limit2(s.tr, r.r0.x, s.k, vn); r.r1.y = rectify_limit2(s.tg, r.r0.y, s.k, vn); r.r1.z = rectify_limit2(s.tb, r.r0.z, s.k, vn);
	return r;
}

// The window statistics at pixel (px, py) of the current call's images; `img` answers x0(i), x1(i), x2(i), xa(i) for the row-major pixel index i, o is
// the current camera's origin.  Not a hit: k = 0 and nothing else is computed.  The taps are visited row by row, dy outside, dx inside, the centre
// included: the order of the sums is part of the definition.
template <class Img> ADYPT_HOST_DEVICE RectifyStats rectify_window(const Img &img, int width, int height, int px, int py, int radius, const float *o)
{
	const int p = py * width + px;
	const Dn4 c1 = img.x1(p);
	RectifySums s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
	if(!(c1.w != 0.0f)) return rectify_finish(s);
	const RectifyCentre c = rectify_centre(c1, img.x2(p), img.xa(p), o);
	for(int dy = -radius; dy <= radius; ++dy)
		for(int dx = -radius; dx <= radius; ++dx)
		{
			const int qx = px + dx, qy = py + dy;
			if(qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
			const int q = qy * width + qx;
			const Dn4 q1 = img.x1(q), q2 = img.x2(q), qa = img.xa(q), q0 = img.x0(q);
			rectify_tap(c, s, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, qa.x, qa.y, qa.z, q0.x, q0.y, q0.z, q0.w);
		}
	return rectify_finish(s);
}

// What a rectified merge is given: the pixel's R0 and R1, and gamma.  on = false: the merge is the plain one to the bit.
struct Rectify { bool on = false; Dn4 r0{0.0f, 0.0f, 0.0f, 0.0f}, r1{0.0f, 0.0f, 0.0f, 0.0f}; float gamma = kRectifyDefaultGamma; };

// one channel: the history value h held against mu within lim; returns f_c, the share of its length the channel leaves the history
ADYPT_HOST_DEVICE float rectify_channel(float *h, float mu, float lim)
{
	const float d = fabsf(*h - mu);
	if(d <= lim) return 1.0f;
	*h = *h < mu ? mu - lim : mu + lim;
	return lim / d;
}

// The history (hr, hg, hb) of a pixel whose window has at least kRectifyMinTaps taps, rectified in place; returns f = min(f_r, f_g, f_b), which the
// history length is multiplied by.  A limit or a distance that is a NaN (a window whose sums overflowed) leaves f = 0: no history.
ADYPT_HOST_DEVICE float rectify_history(const Rectify &rect, float *hr, float *hg, float *hb)
{
	const float fr = rectify_channel(hr, rect.r0.x, rect.gamma * sqrtf(rect.r1.x));
	const float fg = rectify_channel(hg, rect.r0.y, rect.gamma * sqrtf(rect.r1.y));
	const float fb = rectify_channel(hb, rect.r0.z, rect.gamma * sqrtf(rect.r1.z));
	float f = fr;
	f = fg < f ? fg : f;
	f = fb < f ? fb : f;
	if(!(fr >= 0.0f && fg >= 0.0f && fb >= 0.0f)) f = 0.0f;
	return f;
}

}  // namespace adypt
