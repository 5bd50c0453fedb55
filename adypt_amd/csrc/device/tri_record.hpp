// The device triangle record: THE definition of how the reference's 100-byte Triangle becomes the 128-byte record the kernels read (shade.hpp), and of
// the two words that are derived from its material on the way.  Compiled by the host (adypt_create's upload in scene_upload.hpp, adypt_pack_triangles in
// host/host_api.cpp) and by the device (k_pack_triangles, geometry.hip), which therefore give the same bytes: no HIP needed, words are moved, never
// converted.  Restated in numpy as tests/tri_record_truth.py.
//
// Source, 25 words:  0..17 positions and normals | 18..23 texture coordinates | 24 material id
// Record, 32 words:  0..17 positions and normals | 18 material id | 19 class word | 20..25 texture coordinates | 26..31 zero
#pragma once
#include <cstdint>

#ifndef ADYPT_HOST_DEVICE
#ifdef __HIPCC__
#define ADYPT_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define ADYPT_HOST_DEVICE inline
#endif
#endif

namespace adypt {

constexpr int kTriSourceBytes = 100, kTriSourceWords = 25; // Triangle (src/Util/Shape.hpp:70-74)
constexpr int kTriRecordWords = 32;                        // kTriFloat4 x float4 (shade.hpp)
constexpr int kMatSourceBytes = 64, kMatSourceWords = 16;  // GPUMaterial (src/Tracer/OglScene.hpp:19-28)
// words of a material, in the reference's 64 bytes and so in the device's kMatFloat4 record, which begins with them
constexpr int kMatWordDiffuseTex = 0, kMatWordIllum = 12, kMatWordShininess = 13;
constexpr uint8_t kTriClassNoMaterial = 5;                 // the class byte of a triangle whose material id is outside [0, n_mats)

// Shading class of a material = which code of Render() a path that hits it runs (pathtracer.glsl:144-201) — only a SORT KEY for
// k_shade's in-workgroup binning, never an input of the arithmetic.  0 is the key of a miss, 7 of a thread without a path (shade.hpp).
ADYPT_HOST_DEVICE uint32_t material_class(int illum, float shininess, bool textured)
{
	if(illum == 2 && shininess * 0.01f > 0.3f) return textured ? 4u : 3u; // glossy lobe: two canon_pow + sincos
	if(illum == 1 || illum == 2) return textured ? 2u : 1u;                // diffuse lobe
	if(illum == 6 || illum == 7) return 6u;                                // dielectric
	return 5u;                                                             // mirror (3..5) and pass-through (0, 8+)
}

// what a triangle takes from its material
struct TriMaterialWords {
	uint32_t class_word; // word 19 of the record: 1 = a hit here runs the glossy lobe or the dielectric branch of Render() — what k_path's shading rounds
	                     // defer to a round of their own (path.hpp).  A grouping hint only: never an input of the arithmetic.
	uint8_t class_byte;  // k_shade's sort key (ADYPT_SHADE_BIN=1)
};

// `material`: the words of material `matid` (read only where the id is inside [0, n_mats)); n_textures: of the scene
ADYPT_HOST_DEVICE TriMaterialWords tri_material_words(int32_t matid, int64_t n_mats, int32_t n_textures, const uint32_t *material)
{
	TriMaterialWords w{0u, kTriClassNoMaterial};
	if(matid < 0 || matid >= n_mats) return w;
	const int32_t dtex = (int32_t)material[kMatWordDiffuseTex], illum = (int32_t)material[kMatWordIllum];
	float shininess;
	__builtin_memcpy(&shininess, &material[kMatWordShininess], 4);
	const uint32_t cls = material_class(illum, shininess, false);
	w.class_word = (cls == 3u || cls == 6u) ? 1u : 0u;
	w.class_byte = (uint8_t)material_class(illum, shininess, n_textures != 0 && dtex >= 0 && dtex < n_textures);
	return w;
}

// word `k` (0..31) of the record of a triangle whose 25 source words are src[0..24]
ADYPT_HOST_DEVICE uint32_t tri_record_word(const uint32_t *src, int k, uint32_t class_word)
{
	if(k < 18) return src[k];
	if(k == 18) return src[24];
	if(k == 19) return class_word;
	if(k < 26) return src[k - 2];
	return 0u;
}

// The inverse, for readers of the records (adypt_read_triangle_records): source word `k` (0..24) of a record
ADYPT_HOST_DEVICE uint32_t tri_source_word(const uint32_t *rec, int k)
{
	return k < 18 ? rec[k] : k < 24 ? rec[k + 2] : rec[18];
}

}  // namespace adypt
