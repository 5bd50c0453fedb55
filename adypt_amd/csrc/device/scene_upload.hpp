// HBM residency of the scene: what adypt_create uploads, and in which layout the kernels read it.  A section of tracer.hip (included there
// only, after context.hpp, upload() and k_expand_references): every function is one step of adypt_create and returns its error code.
#pragma once
#include "context.hpp"
#include "../../../include/adypt_host.h"

#include <cstring>

namespace {

constexpr long kRefTrianglesAutoMaxMB = 1l << 20; // ADYPT_REF_TRIANGLES_MAX_MB unset: the per-reference triangle copy is made whatever its size

int upload_woop(adypt_ctx *c, const adypt_scene_desc *d)
{
	std::vector<float> woop;
	const float *wp = d->woop;
	if(!wp) { woop.resize((size_t)d->n_refs * 12); adypt_woop_matrices(d->triangles, d->tri_indices, d->n_refs, woop.data()); wp = woop.data(); }
	return upload(c, &c->d_woop, wp, (size_t)d->n_refs * 12);
}

int upload_triangles(adypt_ctx *c, const adypt_scene_desc *d)
{
	// 100-byte Triangle -> 128-byte device record: tri_record.hpp
	std::vector<float> packed((size_t)d->n_tris * kTriFloat4 * 4, 0.0f);
	TRY_CREATE(adypt_pack_triangles(d->triangles, d->n_tris, d->materials, d->n_mats, d->n_textures, packed.data(), nullptr) == ADYPT_OK ? ADYPT_OK
	           : fail(c, ADYPT_E_INVALID, "adypt_create: the triangles could not be packed"));
	return upload(c, &c->d_triangles, packed.data(), packed.size());
}

int upload_shade_classes(adypt_ctx *c, const adypt_scene_desc *d)
{
	// k_shade's sort key per triangle (shade.hpp: material_class).  Off unless ADYPT_SHADE_BIN=1: measured +10 % k_shade time on both
	// bench scenes (profiles/r3_ablations_k_trace.txt item 9) — the kernel waits on its gathers, not on divergent vector-ALU work
	if(!c->tun.shade_bin) return ADYPT_OK;
	std::vector<uint8_t> cls((size_t)std::max<int64_t>(d->n_tris, 1), (uint8_t)5);
	if(adypt_pack_triangles(d->triangles, d->n_tris, d->materials, d->n_mats, d->n_textures, nullptr, cls.data()) != ADYPT_OK)
		return fail(c, ADYPT_E_INVALID, "adypt_create: the triangles could not be classified");
	return upload(c, &c->d_tri_class, cls.data(), cls.size());
}

int upload_textures_and_materials(adypt_ctx *c, const adypt_scene_desc *d)
{
	// textures: RGB8 -> RGBA8 words, every row w + 1 texels long — the extra one repeats the row's first texel, so the horizontal
	// neighbour of the last column (GL_REPEAT) sits next to it and sample_texture fetches a row's two texels in one 8-byte load
	std::vector<uint32_t> texels;
	std::vector<int32_t> desc;
	for(int t = 0; t < d->n_textures; ++t)
	{
		const adypt_texture &tx = d->textures[t];
		if(tx.width <= 0 || tx.height <= 0 || !tx.rgb) return fail(c, ADYPT_E_INVALID, "adypt_create: bad texture " + std::to_string(t));
		desc.push_back((int32_t)texels.size()); desc.push_back(tx.width); desc.push_back(tx.height); desc.push_back(0);
		const size_t base = texels.size(), row = (size_t)tx.width + 1;
		if(base + row * (size_t)tx.height >= ((size_t)1 << 31)) return fail(c, ADYPT_E_INVALID, "adypt_create: more than 2^31 texels");
		texels.resize(base + row * (size_t)tx.height);
		for(int y = 0; y < tx.height; ++y)
		{
			uint32_t *o = texels.data() + base + row * (size_t)y;
			const uint8_t *in = tx.rgb + (size_t)y * tx.width * 3;
			for(int x = 0; x < tx.width; ++x) o[x] = (uint32_t)in[x * 3] | (uint32_t)in[x * 3 + 1] << 8 | (uint32_t)in[x * 3 + 2] << 16 | 0xff000000u;
			o[tx.width] = o[0];
		}
	}
	TRY_CREATE(upload(c, &c->d_texels, texels.data(), texels.size()));
	c->n_texels = (int64_t)texels.size(); c->tex_desc = desc; // (what adypt_update_texture and adypt_read_texels go by: appearance.hip)
	// materials: the reference's 64 bytes + the descriptor of the diffuse texture (one fetch less per textured hit)
	std::vector<uint8_t> mats((size_t)std::max<int64_t>(d->n_mats, 1) * kMatFloat4 * 16, 0);
	for(int64_t m = 0; m < d->n_mats; ++m)
	{
		uint8_t *o = mats.data() + (size_t)m * kMatFloat4 * 16;
		memcpy(o, (const uint8_t *)d->materials + (size_t)m * 64, 64);
		int32_t dtex; memcpy(&dtex, o, 4);
		if(dtex >= 0 && dtex < d->n_textures) memcpy(o + 64, desc.data() + (size_t)dtex * 4, 16);
	}
	return upload(c, &c->d_materials, mats.data(), mats.size());
}

// whether a context with n_refs references keeps the per-reference copy of the records, and its size
bool wants_reference_triangles(const adypt_ctx *c, int64_t n_refs, size_t *bytes)
{
	*bytes = std::max<size_t>((size_t)n_refs * kTriFloat4, 1) * sizeof(float4);
	const long max_mb = c->tun.ref_triangles_max_mb >= 0 ? c->tun.ref_triangles_max_mb : kRefTrianglesAutoMaxMB;
	return max_mb != 0 && (*bytes >> 20) <= (size_t)max_mb; // (0 = never, whatever the size: the tests' way into the remap path with scenes of a few triangles)
}

int make_reference_triangles(adypt_ctx *c)
{
	// k_path looks a hit's triangle up by reference index in a second copy of the records (path.hpp): made here, once, so that nothing is
	// allocated while frames are traced.  Above the size threshold, or when the memory cannot be had, k_path applies the 4-byte
	// uTriIndices remap (traversal.glsl:253-254) in its shading round instead — same image.
	const size_t n16 = (size_t)c->n_refs * kTriFloat4;
	size_t bytes;
	if(wants_reference_triangles(c, c->n_refs, &bytes))
	{
		if(c->d_ref_triangles.alloc(bytes) != hipSuccess) (void)hipGetLastError(); // (left empty)
		else if(n16)
		{
			hipLaunchKernelGGL(k_expand_references, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, c->stream, (const float4 *)c->d_triangles, (const int32_t *)c->d_tri_indices, (size_t)c->n_refs, (float4 *)c->d_ref_triangles);
			HIP_TRY(c, hipGetLastError());
		}
	}
	return ADYPT_OK;
}

int upload_scene(adypt_ctx *c, const adypt_scene_desc *d)
{
	TRY_CREATE(upload(c, &c->d_nodes, (const uint8_t *)d->nodes, (size_t)d->n_nodes * 80));
	TRY_CREATE(upload(c, &c->d_tri_indices, d->tri_indices, (size_t)d->n_refs));
	TRY_CREATE(upload_woop(c, d));
	TRY_CREATE(upload_triangles(c, d));
	TRY_CREATE(upload_shade_classes(c, d));
	TRY_CREATE(upload_textures_and_materials(c, d));
	TRY_CREATE(upload(c, &c->d_local_blocks, c->local_blocks.data(), c->local_blocks.size()));
	TRY_CREATE(make_reference_triangles(c));
	return ctx_refresh_root_card(c);
}

}  // namespace
