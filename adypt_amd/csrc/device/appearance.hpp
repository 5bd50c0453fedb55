// What a surface looks like on the device: THE definition of the material record and of the texture arena, as tri_record.hpp is of the triangle record.
// Compiled by the host (adypt_pack_appearance in host/host_api.cpp, adypt_set_materials' table in appearance.hip) and by the device (k_pack_texels,
// k_tri_attributes in appearance.hip), which therefore give the same bytes: no HIP needed, words are moved, never converted.  Restated in numpy as
// tests/appearance_truth.py.
//
// Material record, 20 words:  0..15 the reference's 64-byte GPUMaterial | 16..19 (texel offset, w, h, 0) of its diffuse texture where 0 <= dtex <
//                             n_textures, else zero
// Texture arena, words:       texture after texture in index order, back to back; a texture is h rows of w + 1 words, word x < w of a row the texel
//                             r | g << 8 | b << 16 | 0xff000000, word w a copy of the row's word 0 (GL_REPEAT's neighbour of the last column; texture.hpp)
// Descriptor, 4 words:        (offset of the texture's first word in the arena, w, h, 0).  The arena stays below 2^31 words.
// A triangle's class word and class byte come from its material by tri_material_words (tri_record.hpp).
#pragma once
#include "tri_record.hpp"
#include <cstdint>

namespace adypt {

constexpr int kMatRecordWords = 20, kMatRecordBytes = 80; // kMatFloat4 x float4 (shade.hpp)
constexpr int kTexDescWords = 4;
constexpr int64_t kMaxArenaWords = (int64_t)1 << 31;      // exclusive
// words of a record that a triangle has from its attributes: 18 material id | 19 class word | 20..25 texture coordinates
constexpr int kTriWordMaterial = 18, kTriWordClass = 19, kTriWordTexcoords = 20, kTriTexcoordWords = 6;

ADYPT_HOST_DEVICE uint32_t texel_word(uint32_t r, uint32_t g, uint32_t b) { return r | g << 8 | b << 16 | 0xff000000u; }

// words a w x h texture takes in the arena
ADYPT_HOST_DEVICE int64_t texture_words(int32_t w, int32_t h) { return ((int64_t)w + 1) * (int64_t)h; }

// where source pixel p (row-major, 0 .. w h - 1) of a texture goes: its word in the texture's part of the arena, and whether it is a row's first pixel,
// which goes to that row's word w as well
ADYPT_HOST_DEVICE uint32_t texel_place(uint32_t p, uint32_t w, bool *wraps)
{
	const uint32_t y = p / w, x = p - y * w;
	*wraps = x == 0u;
	return y * (w + 1u) + x;
}

// word k (0..19) of the record of a material whose 16 source words are src[0..15]; desc: n_textures descriptors
ADYPT_HOST_DEVICE uint32_t material_record_word(const uint32_t *src, int k, int32_t n_textures, const int32_t *desc)
{
	if(k < kMatSourceWords) return src[k];
	const int32_t dtex = (int32_t)src[kMatWordDiffuseTex];
	return dtex >= 0 && dtex < n_textures ? (uint32_t)desc[(int64_t)dtex * kTexDescWords + (k - kMatSourceWords)] : 0u;
}

// The descriptors of n textures given by their sizes (wh: n pairs of width, height) and the arena's length.  The reason a set is refused, or null.
inline const char *appearance_describe(const int32_t *wh, int32_t n, int32_t *desc, int64_t *arena_words)
{
	int64_t at = 0;
	for(int32_t t = 0; t < n; ++t)
	{
		const int32_t w = wh[2 * t], h = wh[2 * t + 1];
		if(w <= 0 || h <= 0) return "a texture's width and height must be positive";
		desc[t * kTexDescWords] = (int32_t)at; desc[t * kTexDescWords + 1] = w; desc[t * kTexDescWords + 2] = h; desc[t * kTexDescWords + 3] = 0;
		at += texture_words(w, h);
		if(at >= kMaxArenaWords) return "more than 2^31 texels";
	}
	*arena_words = at;
	return nullptr;
}

}  // namespace adypt
