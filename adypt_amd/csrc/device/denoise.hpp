// The denoiser: an edge-avoiding a-trous wavelet filter (the spatial half of SVGF) over the albedo-demodulated radiance, guided by the primary hit's
// normal, position and hit flag, its luminance edge-stopping scaled by the variance the noise statistics hold — the variance is filtered along.
// THE definition for host and device (no HIP needed: a host compiler may include it; tests/test_denoise_definition.py does, with
// -ffp-contract=off).  Canonical arithmetic as in noise.hpp: binary32, round to nearest, the operations in the order written, NO fma, no exp / pow —
// only + - * / sqrtf, comparisons and selects — so that a numpy float32 restatement (tests/denoise_truth.py) is bit-exact.
//
// Per pixel p of the W x H image, row-major, four float4 images:  X0 = (D.rgb, V)  the demodulated radiance and the variance of its luminance
//                                                                 X1 = (N.xyz, hit) X2 = (P.xyz, n: read by temporal.hpp only)  XA = (A.rgb, .)
// denoise_prepare makes X0 of level 0, denoise_level makes level i + 1 from level i, denoise_remodulate the result from the last.
#pragma once
#include "noise.hpp"

namespace adypt {

struct Dn4 { float x, y, z, w; };

constexpr int kDenoiseMaxLevels = 6;
constexpr float kDenoiseAlbedoFloor = 0.01f;  // the constants are part of the definition, not tunables
constexpr float kDenoiseSigmaFloor = 1e-4f;
constexpr float kDenoiseDepthFloor = 1e-6f;

struct DenoiseParams { int levels; float sigma_l, sigma_z; };
constexpr DenoiseParams kDenoiseDefaults{5, 4.0f, 0.1f};
// (written so that a NaN sigma is refused)
inline bool denoise_params_valid(const DenoiseParams &p) { return p.levels >= 1 && p.levels <= kDenoiseMaxLevels && p.sigma_l > 0.0f && p.sigma_z > 0.0f; }

// tap weights of the 5-tap B3 spline and of the 3-tap variance prefilter, index = offset + 2 / offset + 1
ADYPT_HOST_DEVICE float denoise_h(int i) { return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }
ADYPT_HOST_DEVICE float denoise_k3(int i) { return i == 1 ? 0.5f : 0.25f; }

// level 0: radiance c (rgb), luminance second moment m2 after n samples (n >= 2), albedo a
ADYPT_HOST_DEVICE Dn4 denoise_prepare(float cr, float cg, float cb, float m2, float n, float ar, float ag, float ab)
{
	const float v = m2 / (n * (n - 1.0f));
	const float la = noise_luminance(ar, ag, ab) + kDenoiseAlbedoFloor;
	Dn4 r;
	r.x = cr / (ar + kDenoiseAlbedoFloor); r.y = cg / (ag + kDenoiseAlbedoFloor); r.z = cb / (ab + kDenoiseAlbedoFloor);
	r.w = v / (la * la);
	return r;
}

// One level at pixel (px, py) with tap distance `step`.  `img` answers x0(i), x1(i), x2(i) for the row-major pixel index i; a tap counts when it
// lies inside the image and its hit flag is the centre's, the others are skipped entirely.
template <class Img> ADYPT_HOST_DEVICE Dn4 denoise_level(const Img &img, int width, int height, int px, int py, int step, float sigma_l, float sigma_z)
{
	const int p = py * width + px;
	const Dn4 c0 = img.x0(p), c1 = img.x1(p), c2 = img.x2(p); // the centre's values stay in registers
	const bool hit = c1.w != 0.0f;
	// 1. the variance, prefiltered over the 3x3 neighbours at distance 1 (whatever the step)
	float gs = 0.0f, gw = 0.0f;
	for(int dy = -1; dy <= 1; ++dy)
		for(int dx = -1; dx <= 1; ++dx)
		{
			const int qx = px + dx, qy = py + dy;
			if(qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
			const int q = qy * width + qx;
			if(img.x1(q).w != c1.w) continue;
			const float k = denoise_k3(dx + 1) * denoise_k3(dy + 1);
			gs = gs + k * img.x0(q).w;
			gw = gw + k;
		}
	const float g = gs / gw;
	const float sl = sigma_l * sqrtf(g) + kDenoiseSigmaFloor;
	const float yp = noise_luminance(c0.x, c0.y, c0.z);
	// 2. the 5x5 taps at distance `step`
	float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
	for(int dy = -2; dy <= 2; ++dy)
		for(int dx = -2; dx <= 2; ++dx)
		{
			const int qx = px + step * dx, qy = py + step * dy;
			if(qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
			const int q = qy * width + qx;
			const Dn4 q1 = img.x1(q);
			if(q1.w != c1.w) continue;
			const Dn4 q0 = img.x0(q);
			float w;
			if(dx == 0 && dy == 0) w = denoise_h(2) * denoise_h(2);
			else
			{
				float t = 1.0f, wz = 1.0f;
				if(hit)
				{
					const Dn4 q2 = img.x2(q);
					const float d = (c1.x * q1.x + c1.y * q1.y) + c1.z * q1.z;
					t = d > 0.0f ? d : 0.0f; // (a NaN becomes 0)
					t = t * t; t = t * t; t = t * t; t = t * t; t = t * t;
					const float ex = q2.x - c2.x, ey = q2.y - c2.y, ez = q2.z - c2.z;
					const float len = sqrtf((ex * ex + ey * ey) + ez * ez);
					const float pd = fabsf((c1.x * ex + c1.y * ey) + c1.z * ez);
					const float z = 1.0f - pd / (sigma_z * len + kDenoiseDepthFloor);
					wz = z > 0.0f ? z : 0.0f;
				}
				const float xl = fabsf(noise_luminance(q0.x, q0.y, q0.z) - yp) / sl;
				const float wl = 1.0f / (1.0f + xl * xl);
				w = (((denoise_h(dx + 2) * denoise_h(dy + 2)) * t) * wz) * wl;
			}
			sw = sw + w;
			sr = sr + w * q0.x; sg = sg + w * q0.y; sb = sb + w * q0.z;
			sv = sv + (w * w) * q0.w;
		}
	Dn4 r;
	r.x = sr / sw; r.y = sg / sw; r.z = sb / sw;
	r.w = sv / (sw * sw);
	return r;
}

// the result: the filtered demodulated radiance times the albedo it was divided by
ADYPT_HOST_DEVICE void denoise_remodulate(const Dn4 &d, const Dn4 &albedo, float *rgb)
{
	rgb[0] = d.x * (albedo.x + kDenoiseAlbedoFloor); rgb[1] = d.y * (albedo.y + kDenoiseAlbedoFloor); rgb[2] = d.z * (albedo.z + kDenoiseAlbedoFloor);
}

}  // namespace adypt
