// The scene arrays a kernel is launched with and the diffuse texture fetch of FetchInfo (pathtracer.glsl:73-100), in a header of their own: shade.hpp
// (the tracer's unit) and denoise_kernels.hpp (the denoiser's, which follows mirrors and glass to a surface that may be textured) compile the same text.
// Nothing here defines a kernel.
#pragma once
#include "canon_math.hpp"

namespace adypt {

constexpr int kTriFloat4 = 8;                  // device triangle record: 8 x float4 = one 128-byte line
constexpr int kMatFloat4 = 5;                  // device material record: the reference's 64 bytes + (texel offset, w, h, 0) of its diffuse texture

struct SceneArgs {
	const float4 *triangles;       // kTriFloat4 float4 per triangle (repacked, see header)
	const float4 *materials;       // kMatFloat4 x float4 per material
	const uint32_t *texels;        // RGBA8, all textures back to back; every row is followed by a copy of its first texel (w + 1 per row)
	const int32_t *local_blocks;   // global block id of each owned block
	const uint8_t *tri_class;      // per triangle: shading class of its material, 1..6 (material_class); null = k_shade does not bin
};

__device__ __forceinline__ int pos_mod(int a, int n) { int r = a % n; return r < 0 ? r + n : r; }

// GL_LINEAR / GL_REPEAT / RGB8, single level, canonical fp32 weights (see oracle.cpp sample_texture).  d = (texel offset, w, h) from the
// material record.  The two texels of a row come in one 8-byte load: rows are stored w + 1 texels long, the last one a copy of the
// first, so (i0, i0 + 1) is the wrapped pair too — 2 vector-memory instructions per sample instead of 4.
struct __attribute__((packed, aligned(4))) TexelPair { uint32_t a, b; };
__device__ inline F3 sample_texture(const SceneArgs &sc, int4 d, float s, float t)
{
	const int w = d.y, h = d.z;
	const uint32_t *tx = sc.texels + d.x;
	const float uu = fmaf(s, (float)w, -0.5f), vv = fmaf(t, (float)h, -0.5f);
	float fu = floorf(uu), fv = floorf(vv);
	const float a = uu - fu, b = vv - fv;
	fu = gl_min(gl_max(fu, -1e9f), 1e9f); fv = gl_min(gl_max(fv, -1e9f), 1e9f);
	const int i0 = pos_mod((int)fu, w), j0 = pos_mod((int)fv, h);
	const int j1 = j0 + 1 == h ? 0 : j0 + 1;
	const TexelPair r0 = *(const TexelPair *)(tx + (size_t)j0 * (size_t)(w + 1) + i0), r1 = *(const TexelPair *)(tx + (size_t)j1 * (size_t)(w + 1) + i0);
	auto rgb = [](uint32_t p) { return f3(unorm8_to_float(p), unorm8_to_float(p >> 8), unorm8_to_float(p >> 16)); };
	const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
	F3 r = rgb(r0.a) * w00;
	r = fma3(rgb(r0.b), w10, r);
	r = fma3(rgb(r1.a), w01, r);
	r = fma3(rgb(r1.b), w11, r);
	return r;
}

__device__ __forceinline__ F3 textured_diffuse(const SceneArgs &sc, int tri_idx, int4 desc, float u, float v, float w)
{
	const float4 *p = sc.triangles + (size_t)tri_idx * kTriFloat4 + 5;
	const float4 a = p[0], b = p[1]; // tc0.xy tc1.xy | tc2.xy pad
	const float ts = fmaf(b.x, w, fmaf(a.z, v, a.x * u));
	const float tt = fmaf(b.y, w, fmaf(a.w, v, a.y * u));
	return sample_texture(sc, desc, ts, tt);
}

}  // namespace adypt
