// Guides of the first surface that is not a perfect mirror or glass (adypt_denoise_specular): from the primary hit the chain follows the delta
// materials — illum 3..5 reflect, illum 6..7 transmit where they can — for up to K bounces and hands the denoiser the albedo, normal and position of
// the surface it ends on, and a CLASS per pixel that goes where the hit flag went (X1.w): denoise_level counts a tap only when its X1.w is the
// centre's, so pixels of different classes never pool.
// THE definition for host and device (no HIP needed: tests/test_specular_definition.py compiles it with g++ -ffp-contract=off).  Canonical arithmetic
// as in denoise.hpp: binary32, round to nearest, the operations in the order written, NO fma, only + - * / sqrtf, comparisons and selects, so that the
// numpy float32 restatement (tests/specular_truth.py) is bit-exact.
//
// Per pixel, K = bounces in [1, kChainMaxBounces]:
//     primary miss                        class 0, the guides of the primary capture
//     the chain starts at the primary hit with its captured normal and position, d = normalize(P0 - camera origin), T = (1, 1, 1), L = 0
//     at a surface (chain_at_surface)     a material that is not delta — a bad material id, illum 2 at any shininess — ends the chain: L = 0 the captured
//                                         guides, class 1; L > 0 albedo T x Kd (Kd what the shading takes: the diffuse texture where there is one), the
//                                         surface's normal and position, class 1 + L.  A delta material at L == K ends it TRUNCATED: albedo T x S, S = Ks of
//                                         a mirror and (1, 1, 1) of a dielectric, class 1 + L.  Else the next direction: chain_mirror / chain_dielectric
//     the ray (P, ray_tmin, d) is traced to its closest hit.  A miss ends the chain ESCAPED: albedo T, normal d, position (0, 0, 0) — the plane term is
//                                         then 1 and the normal term compares sky directions — class -(L + 1).  A hit is the next surface (chain_hit_point),
//                                         L <- L + 1
// What cannot be normalised.  chain_normalize gives (0, 0, 0) and `false` when the squared length is not a positive number up to kTemporalFiniteMax
// (zero, an infinity, a NaN): the rule of temporal_previous_point.  An interpolated normal of a hit that cannot be normalised IS (0, 0, 0): as the
// guide of a surface that ends the chain it makes every neighbour's normal weight 0; on a mirror d . n = 0 and the ray goes straight on; on a
// dielectric cosi = 0 and the branch below is taken with n = 0.  A direction that cannot be normalised — P0 at the camera origin, a next direction
// that is not finite (a NaN normal of the primary capture, ior 0) — is never traced: the chain ends where it stands as a truncated chain does (at
// L = 0: the captured guides, class 1).  So d is a finite vector whenever a ray is traced, whatever the inputs.
#pragma once
#include "temporal.hpp"

namespace adypt {

constexpr int kChainMaxBounces = 8;
inline bool chain_bounces_valid(int k) { return k >= 1 && k <= kChainMaxBounces; }

struct Ch3 { float x, y, z; };

ADYPT_HOST_DEVICE float chain_dot(const Ch3 &a, const Ch3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// v / |v|; (0, 0, 0) and false where |v|^2 is not in (0, kTemporalFiniteMax]
ADYPT_HOST_DEVICE bool chain_normalize(const Ch3 &v, Ch3 *out)
{
	const float len2 = chain_dot(v, v);
	if(!(len2 > 0.0f && len2 <= kTemporalFiniteMax)) { *out = Ch3{0.0f, 0.0f, 0.0f}; return false; }
	const float len = sqrtf(len2);
	*out = Ch3{v.x / len, v.y / len, v.z / len};
	return true;
}

// a direction the chain may trace: every component finite, the squared length a positive finite number
ADYPT_HOST_DEVICE bool chain_direction_ok(const Ch3 &d)
{
	const float len2 = chain_dot(d, d);
	return len2 > 0.0f && len2 <= kTemporalFiniteMax;
}

ADYPT_HOST_DEVICE bool chain_is_mirror(int illum) { return illum >= 3 && illum <= 5; }
ADYPT_HOST_DEVICE bool chain_is_dielectric(int illum) { return illum == 6 || illum == 7; }
ADYPT_HOST_DEVICE bool chain_is_delta(bool bad_material, int illum) { return !bad_material && illum >= 3 && illum <= 7; }

// the start: the direction the camera sees the primary hit in; false: the chain does not start (class 1)
ADYPT_HOST_DEVICE bool chain_start_direction(const Ch3 &p0, const float *origin, Ch3 *d)
{
	return chain_normalize(Ch3{p0.x - origin[0], p0.y - origin[1], p0.z - origin[2]}, d);
}

// the point and the normal of a hit (u, v) on the triangle record `tri` (words 0..8 the positions, 9..17 the normals): p0 by u, p1 by v, p2 by w
ADYPT_HOST_DEVICE void chain_hit_point(const float *tri, float u, float v, Ch3 *p, Ch3 *n)
{
	const float w = (1.0f - u) - v;
	*p = Ch3{(tri[0] * u + tri[3] * v) + tri[6] * w, (tri[1] * u + tri[4] * v) + tri[7] * w, (tri[2] * u + tri[5] * v) + tri[8] * w};
	const Ch3 m{(tri[9] * u + tri[12] * v) + tri[15] * w, (tri[10] * u + tri[13] * v) + tri[16] * w, (tri[11] * u + tri[14] * v) + tri[17] * w};
	(void)chain_normalize(m, n);
}

ADYPT_HOST_DEVICE Ch3 chain_reflect(const Ch3 &d, const Ch3 &n)
{
	const float k = 2.0f * chain_dot(d, n);
	return Ch3{d.x - k * n.x, d.y - k * n.y, d.z - k * n.z};
}

// illum 3..5: the normal is turned against the ray first
ADYPT_HOST_DEVICE Ch3 chain_mirror(const Ch3 &d, Ch3 n)
{
	if(chain_dot(d, n) > 0.0f) n = Ch3{-n.x, -n.y, -n.z};
	return chain_reflect(d, n);
}

// illum 6, 7: the dielectric branch of the shading with the Fresnel draw taken as "transmit" — refraction where cos2 > 0, else (total internal
// reflection) the mirror direction about the normal as that branch has turned it.  *refracted says which it was.
ADYPT_HOST_DEVICE Ch3 chain_dielectric(const Ch3 &d, Ch3 n, float ior, bool *refracted)
{
	float cosi = chain_dot(d, n);
	float etai, etat;
	if(cosi > 0.0f) { etai = ior; etat = 1.0f; }
	else { etai = 1.0f; etat = ior; n = Ch3{-n.x, -n.y, -n.z}; cosi = -cosi; }
	const float eta = etai / etat;
	const float cos2 = 1.0f - (eta * eta) * (1.0f - cosi * cosi);
	*refracted = cos2 > 0.0f;
	if(!*refracted) return chain_reflect(d, n);
	const float k = eta * cosi + sqrtf(cos2);
	Ch3 r;
	(void)chain_normalize(Ch3{d.x * eta + n.x * k, d.y * eta + n.y * k, d.z * eta + n.z * k}, &r);
	return r;
}

// what a pixel's chain is between two surfaces: 32 bytes with the padding the device keeps it in
struct ChainState { Ch3 t, d; int length; };

// what the material of a surface says to the chain: kd what the shading would take as the diffuse colour (the texture's where there is one); a bad
// material id has illum 0 and kd = ks = (0, 0, 0), as the shading's fetch gives it
struct ChainMaterial { bool bad; int illum; Ch3 kd, ks; float ior; };

// the guides of a pixel whose chain has ended
struct ChainEnd { Ch3 albedo, normal, position; int cls; };

enum ChainVerdict { kChainGoesOn, kChainEnds };

// The chain `s` stands on a surface with material `m`, normal `n`, point `p` (L = s.length bounces behind it, L > 0: for L = 0 see chain_at_primary).
// kChainEnds: *end holds the guides.  kChainGoesOn: s has the next direction and throughput; the caller traces (p, tmin, s.d).
ADYPT_HOST_DEVICE ChainVerdict chain_at_surface(ChainState &s, const ChainMaterial &m, const Ch3 &n, const Ch3 &p, int bounces, ChainEnd *end)
{
	end->normal = n; end->position = p; end->cls = 1 + s.length;
	if(!chain_is_delta(m.bad, m.illum))
	{
		end->albedo = Ch3{s.t.x * m.kd.x, s.t.y * m.kd.y, s.t.z * m.kd.z};
		return kChainEnds;
	}
	const bool mirror = chain_is_mirror(m.illum);
	const Ch3 sm = mirror ? m.ks : Ch3{1.0f, 1.0f, 1.0f};
	end->albedo = Ch3{s.t.x * sm.x, s.t.y * sm.y, s.t.z * sm.z};
	if(s.length >= bounces) return kChainEnds; // truncated
	bool refracted;
	const Ch3 next = mirror ? chain_mirror(s.d, n) : chain_dielectric(s.d, n, m.ior, &refracted);
	if(!chain_direction_ok(next)) return kChainEnds; // (as a truncated chain: see the head)
	s.d = next;
	s.t = end->albedo;
	return kChainGoesOn;
}

// The primary hit: `n`, `p` the captured normal and position guides.  kChainEnds: the pixel keeps the captured guides and has class 1.
ADYPT_HOST_DEVICE ChainVerdict chain_at_primary(ChainState &s, const ChainMaterial &m, const Ch3 &n, const Ch3 &p, const float *origin, int bounces)
{
	s.t = Ch3{1.0f, 1.0f, 1.0f}; s.d = Ch3{0.0f, 0.0f, 0.0f}; s.length = 0;
	if(!chain_is_delta(m.bad, m.illum)) return kChainEnds;
	if(!chain_start_direction(p, origin, &s.d)) return kChainEnds;
	ChainEnd unused;
	return chain_at_surface(s, m, n, p, bounces, &unused);
}

// the traced ray found nothing: the guides of the sky in direction d
ADYPT_HOST_DEVICE ChainEnd chain_escaped(const ChainState &s)
{
	return ChainEnd{s.t, s.d, Ch3{0.0f, 0.0f, 0.0f}, -(s.length + 1)};
}

// ---- the virtual point (adypt_denoise_temporal_specular) ----
// The camera ray unfolded to the chain's full length: of a planar mirror the mirror image of the surface the chain ended on, which stands still in the
// world while the camera moves; the temporal merge reprojects a followed pixel through it (temporal.hpp temporal_merge_virtual).  Through curved mirrors
// and refraction it is only approximate: the merge still holds every tap against the followed guides, so it then finds less history, never another surface.
//     a chain that starts (chain_at_primary: kChainGoesOn)   len = chain_start_length(P0, O): the very `len` of chain_start_direction
//     at every later hit                                     len <- chain_unfold(len, the hit point of chain_hit_point, the origin of the ray that found it)
//     a chain that ends on a surface (class 1 + L, L >= 1, truncated chains too)   chain_virtual_point(P0, O, len), P0 the primary position guide
// Who has none: class 1 pixels are their own virtual point (Pv = P, valid); classes <= 0 (a primary miss, an escaped chain) have no virtual point.

ADYPT_HOST_DEVICE float chain_start_length(const Ch3 &p0, const float *origin)
{
	const Ch3 e{p0.x - origin[0], p0.y - origin[1], p0.z - origin[2]};
	return sqrtf(chain_dot(e, e));
}

ADYPT_HOST_DEVICE float chain_unfold(float len, const Ch3 &hit, const Ch3 &ray_origin)
{
	const Ch3 e{hit.x - ray_origin.x, hit.y - ray_origin.y, hit.z - ray_origin.z};
	return len + sqrtf(chain_dot(e, e));
}

// valid: len is a positive number up to kTemporalFiniteMax (an infinity and a NaN are refused); p is computed either way
struct ChainVirtual { Ch3 p; bool valid; };

ADYPT_HOST_DEVICE ChainVirtual chain_virtual_point(const Ch3 &p0, const float *origin, float len)
{
	Ch3 d0;
	(void)chain_start_direction(p0, origin, &d0);
	return ChainVirtual{Ch3{origin[0] + d0.x * len, origin[1] + d0.y * len, origin[2] + d0.z * len}, len > 0.0f && len <= kTemporalFiniteMax};
}

}  // namespace adypt
