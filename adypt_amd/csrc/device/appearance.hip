// Changing what the surfaces look like on the device (include/adypt_hip.h adypt_set_materials, adypt_update_texture, adypt_set_triangle_attributes; the
// definition: appearance.hpp).  A translation unit of its own: nothing here is part of the tracer's code object, and the context is reached through
// ctx_access.hpp only.  What a call runs, all on the context's stream after the context has been drained:
//     the staging copies  the caller's RGB8 bytes, texture after texture as they are; the material ids (4 B) and texture coordinates (24 B) per triangle
//     k_pack_texels       RGB8 -> the padded RGBA8 rows of the arena, one launch for all textures of a call.  A workgroup takes 256 consecutive SOURCE
//                         pixels of one texture: 768 contiguous bytes at any byte alignment, which it reads as the at most 193 aligned words that hold
//                         them, neighbouring lanes neighbouring words, into LDS.  Lane i then takes its three bytes from LDS and writes word
//                         y (w + 1) + x: neighbouring lanes neighbouring words but for the one skipped at a row's end, which the row's first pixel
//                         writes as well (the wrap texel).  No lane fetches single bytes from memory or walks it at a 3-byte stride.
//     k_tri_attributes    one thread per triangle of a range: words 18 and 19 read and written as one 8-byte vector (the id where ids are given, the
//                         class word always, from the table as it is then), words 20..25 as a 16-byte and an 8-byte store where texture coordinates are
//                         given, the class byte where the context keeps one; the triangles whose class word changed are counted by one atomic per wave.
//     k_ref_attributes    three threads per reference, 16 bytes each: the 48 bytes that hold words 18..25 of its triangle's record, into the per-reference
//                         copy where the context keeps one (Appearance, for why not k_expand_references).
// adypt_set_materials builds the new table and arena in NEW buffers, reclassifies the triangles from them, and only then lets the context take them
// (ctx_replace_appearance): what can fail comes before anything of the context is written.
#include "ctx_unit.hpp"
#include "appearance.hpp"
#include "../../../include/adypt_hip.h"

#include <cstring>
#include <string>
#include <vector>

using namespace adypt;

namespace {

constexpr int kLookThreads = 256;                                  // = source pixels per workgroup of k_pack_texels, triangles of k_tri_attributes
constexpr int kTileWords = (3 + 3 * kLookThreads + 3) / 4;         // 193: the aligned words that hold 768 bytes at any byte alignment
constexpr int kRecordVecs = kTriRecordWords / 4;                   // 8 x 16 bytes per record
constexpr int kAppearanceStages = 3;                               // adypt_get_appearance: staged, packed, classified
static_assert(kTileWords <= kLookThreads, "a workgroup loads its tile with one word per lane");
static_assert(kTriWordMaterial == 18 && kTriWordClass == 19 && kTriWordTexcoords == 20 && kTriTexcoordWords == 6, "the vectors k_tri_attributes and k_ref_attributes move");

// one texture of a launch of k_pack_texels; the list ends with an entry whose first_tile is the number of workgroups
struct TexelJob {
	int64_t src_byte;     // where its w x h x 3 bytes begin in the staging buffer
	uint32_t out_word;    // where its (w + 1) x h words begin in the arena
	uint32_t w, n_px;     // n_px = w h
	uint32_t first_tile;  // the first workgroup of the texture: it has ceil(n_px / 256)
};

// stage: the staged bytes as words, readable up to the word that holds the last staged byte; jobs: n_jobs + 1 entries
__global__ __launch_bounds__(kLookThreads) void k_pack_texels(const uint32_t *__restrict__ stage, const TexelJob *__restrict__ jobs, int n_jobs, uint32_t *__restrict__ arena)
{
	__shared__ uint32_t s_src[kTileWords + 1]; // (+ 1: the last lane's two-word window)
	const uint32_t tid = threadIdx.x, tile = blockIdx.x;
	int lo = 0, hi = n_jobs; // the job whose tiles hold this one: jobs[lo].first_tile <= tile < jobs[lo + 1].first_tile
	while(hi - lo > 1)
	{
		const int mid = (lo + hi) >> 1;
		if(jobs[mid].first_tile <= tile) lo = mid; else hi = mid;
	}
	const TexelJob job = jobs[lo];
	const uint32_t p0 = (tile - job.first_tile) * (uint32_t)kLookThreads;
	const uint32_t count = job.n_px - p0 < (uint32_t)kLookThreads ? job.n_px - p0 : (uint32_t)kLookThreads;
	const int64_t begin = job.src_byte + 3 * (int64_t)p0;
	const uint32_t mis = (uint32_t)(begin & 3), n_words = (mis + 3u * count + 3u) >> 2;
	if(tid < n_words) s_src[tid] = stage[(begin >> 2) + tid];
	if(tid == n_words) s_src[tid] = 0u; // (looked at by the last lane's window, never used)
	__syncthreads();
	if(tid >= count) return;
	const uint32_t o = mis + 3u * tid, k = o >> 2, sh = (o & 3u) * 8u;
	const uint32_t rgb = (uint32_t)((((uint64_t)s_src[k + 1] << 32) | s_src[k]) >> sh);
	const uint32_t word = texel_word(rgb & 0xffu, (rgb >> 8) & 0xffu, (rgb >> 16) & 0xffu);
	bool wraps;
	const uint32_t at = job.out_word + texel_place(p0 + tid, job.w, &wraps);
	arena[at] = word;
	if(wraps) arena[at + job.w] = word;
}

// records: n_tris x 128 bytes, of which [first, first + count) are rewritten; ids: count words or null; texcoords: count x 6 floats or null;
// materials: n_mats records of mat_words words; classes: n_tris bytes or null; changed: one word, cleared by the caller
__global__ __launch_bounds__(kLookThreads) void k_tri_attributes(uint4 *records, int64_t first, int64_t count, const int32_t *__restrict__ ids, const float2 *__restrict__ texcoords,
                                                                 const uint32_t *__restrict__ materials, int mat_words, int64_t n_mats, int n_textures, uint8_t *classes, uint32_t *changed)
{
	const int64_t i = (int64_t)blockIdx.x * kLookThreads + threadIdx.x;
	const bool live = i < count;
	bool differs = false;
	if(live)
	{
		const size_t t = (size_t)(first + i);
		uint4 *rec = records + t * kRecordVecs;
		uint2 *rec2 = (uint2 *)rec;
		const uint2 was = rec2[kTriWordMaterial / 2];
		const int32_t matid = ids ? ids[i] : (int32_t)was.x;
		const bool known = matid >= 0 && matid < n_mats;
		const TriMaterialWords w = tri_material_words(matid, n_mats, n_textures, materials + (known ? (size_t)matid * mat_words : 0));
		differs = w.class_word != was.y;
		rec2[kTriWordMaterial / 2] = make_uint2((uint32_t)matid, w.class_word);
		if(classes) classes[t] = w.class_byte;
		if(texcoords)
		{
			const float2 a = texcoords[3 * i], b = texcoords[3 * i + 1], c = texcoords[3 * i + 2];
			((float4 *)rec)[kTriWordTexcoords / 4] = make_float4(a.x, a.y, b.x, b.y);
			((float2 *)rec)[(kTriWordTexcoords + 4) / 2] = c;
		}
	}
	const unsigned long long mask = __ballot(differs);
	if((threadIdx.x & 63) == 0 && mask) atomicAdd(changed, (uint32_t)__popcll(mask));
}

// the per-reference copy follows: float4 4, 5 and 6 of a record hold words 16..27, of which 16 and 17 are the normal's and 26, 27 zero in both.  Three
// lanes per reference, one vector each: neighbouring lanes write neighbouring 16 bytes of the 48
__global__ __launch_bounds__(kLookThreads) void k_ref_attributes(float4 *ref, const float4 *__restrict__ records, const int32_t *__restrict__ tri_indices, int64_t n_refs, int64_t first, int64_t count)
{
	const int64_t g = (int64_t)blockIdx.x * kLookThreads + threadIdx.x, r = g / 3;
	if(r >= n_refs) return;
	const int q = 4 + (int)(g - 3 * r);
	const int64_t t = tri_indices[r];
	if(t < first || t >= first + count) return;
	ref[(size_t)r * kRecordVecs + q] = records[(size_t)t * kRecordVecs + q];
}

// kept per context: the staging buffers, at their largest, and what the last call did
struct Appearance {
	Buffer<uint32_t> stage;       // RGB8 bytes of a call's textures, then nothing: 3 B per texel
	Buffer<TexelJob> jobs;
	Buffer<int32_t> ids;          // 4 B per triangle of a range
	Buffer<float2> texcoords;     // 24 B per triangle of a range
	Buffer<uint32_t> changed;
	StageTimer<kAppearanceStages + 1> timer;
	int64_t reclassed = 0;
	size_t device_bytes() const { return stage.bytes() + jobs.bytes() + ids.bytes() + texcoords.bytes() + changed.bytes(); }
};

// the textures of one launch of k_pack_texels
struct TexelPlan {
	std::vector<TexelJob> jobs;   // + the closing entry
	std::vector<const uint8_t *> rgb;
	int64_t src_bytes = 0;
	size_t stage_words() const { return (size_t)((src_bytes + 3) / 4) + 1; }
	void add(const uint8_t *pixels, int32_t w, int32_t h, uint32_t out_word)
	{
		const uint32_t n_px = (uint32_t)w * (uint32_t)h, first_tile = jobs.empty() ? 0u : jobs.back().first_tile + grid_of(jobs.back().n_px, kLookThreads);
		jobs.push_back(TexelJob{src_bytes, out_word, (uint32_t)w, n_px, first_tile});
		rgb.push_back(pixels);
		src_bytes += 3 * (int64_t)n_px;
	}
	uint32_t close()
	{
		const uint32_t tiles = jobs.empty() ? 0u : jobs.back().first_tile + grid_of(jobs.back().n_px, kLookThreads);
		jobs.push_back(TexelJob{src_bytes, 0u, 1u, 0u, tiles});
		return tiles;
	}
};

// room for a plan's staging: everything that can fail for want of memory
int reserve_texels(adypt_ctx *c, Appearance &a, const TexelPlan &plan)
{
	CTX_TRY(c, at_least(a.stage, plan.stage_words()));
	CTX_TRY(c, at_least(a.jobs, plan.jobs.size()));
	return ADYPT_OK;
}

// the staging copies and the launch of a closed plan, between marks 0, 1 and 2 of the timer
int pack_texels(adypt_ctx *c, Appearance &a, const TexelPlan &plan, uint32_t tiles, uint32_t *arena, hipStream_t stream)
{
	CTX_TRY(c, a.timer.mark(0, stream));
	for(size_t t = 0; t + 1 < plan.jobs.size(); ++t)
		CTX_TRY(c, hipMemcpyAsync((uint8_t *)a.stage.get() + plan.jobs[t].src_byte, plan.rgb[t], 3 * (size_t)plan.jobs[t].n_px, hipMemcpyHostToDevice, stream));
	if(tiles) CTX_TRY(c, hipMemcpyAsync(a.jobs.get(), plan.jobs.data(), plan.jobs.size() * sizeof(TexelJob), hipMemcpyHostToDevice, stream));
	CTX_TRY(c, a.timer.mark(1, stream));
	if(tiles)
	{
		hipLaunchKernelGGL(k_pack_texels, dim3(tiles), dim3(kLookThreads), 0, stream, (const uint32_t *)a.stage.get(), (const TexelJob *)a.jobs.get(), (int)plan.jobs.size() - 1, arena);
		CTX_TRY(c, hipGetLastError());
	}
	CTX_TRY(c, a.timer.mark(2, stream));
	return ADYPT_OK;
}

// k_tri_attributes over [first, first + count) against the table given, then the per-reference copy: behind mark 2, in front of mark 3.  ids and
// texcoords: staged already, or null
int write_attributes(adypt_ctx *c, Appearance &a, int64_t first, int64_t count, const int32_t *ids, const float2 *texcoords, const float4 *materials, int64_t n_mats, int n_textures,
                     hipStream_t stream)
{
	const CtxScene sc = ctx_scene(c);
	const CtxAppearance ap = ctx_appearance(c);
	CTX_TRY(c, hipMemsetAsync(a.changed.get(), 0, sizeof(uint32_t), stream));
	if(count > 0)
	{
		hipLaunchKernelGGL(k_tri_attributes, dim3(grid_of(count, kLookThreads)), dim3(kLookThreads), 0, stream, (uint4 *)sc.triangles, first, count, ids, texcoords,
		                   (const uint32_t *)materials, ap.mat_float4 * 4, n_mats, n_textures, ap.tri_class, a.changed.get());
		CTX_TRY(c, hipGetLastError());
		if(ap.expand_whole) CTX_STEP(ctx_expand_references(c)); // (measurement only, tools/appearance_cost.py: the same bytes)
		else if(ap.ref_triangles && sc.n_refs > 0)
		{
			hipLaunchKernelGGL(k_ref_attributes, dim3(grid_of(3 * sc.n_refs, kLookThreads)), dim3(kLookThreads), 0, stream, ap.ref_triangles, (const float4 *)sc.triangles, sc.tri_indices,
			                   sc.n_refs, first, count);
			CTX_TRY(c, hipGetLastError());
		}
	}
	CTX_TRY(c, a.timer.mark(3, stream));
	return ADYPT_OK;
}

// the end of every setter: the stream waited for, the count read, the accumulation started again as adypt_update_triangles starts it
int finish(adypt_ctx *c, Appearance &a, hipStream_t stream, bool counted)
{
	uint32_t changed = 0;
	if(counted) CTX_TRY(c, hipMemcpyAsync(&changed, a.changed.get(), sizeof(changed), hipMemcpyDeviceToHost, stream));
	CTX_TRY(c, hipStreamSynchronize(stream));
	a.reclassed = (int64_t)changed;
	a.timer.complete();
	return adypt_reset(c); // the image, the frozen blocks, the frames parked ahead and the primary-hit cache were the old surfaces'
}

bool layouts_fit(adypt_ctx *c)
{
	return ctx_scene(c).tri_float4 == kRecordVecs && ctx_appearance(c).mat_float4 * 4 == kMatRecordWords;
}

}  // namespace

extern "C" {

int adypt_set_materials(adypt_ctx *c, const void *materials, int64_t n_mats, const adypt_texture *textures, int32_t n_textures)
{
	if(!c) return ADYPT_E_INVALID;
	const std::string who = "adypt_set_materials: ";
	if(n_mats < 0) return ctx_fail(c, ADYPT_E_INVALID, who + "n_mats is negative");
	if(n_mats > 0 && !materials) return ctx_fail(c, ADYPT_E_INVALID, who + "materials is null");
	const bool keep = n_textures == -1 && !textures;
	if(!keep && (n_textures < 0 || (n_textures > 0 && !textures))) return ctx_fail(c, ADYPT_E_INVALID, who + "textures is null or n_textures negative (NULL with -1 keeps the textures)");
	if(!layouts_fit(c)) return ctx_fail(c, ADYPT_E_HIP, who + "the record layouts are not appearance.hpp's");
	// the new descriptors and the plan of the one texel launch
	std::vector<int32_t> desc;
	int64_t arena_words = 0;
	TexelPlan plan;
	if(!keep)
	{
		std::vector<int32_t> wh((size_t)n_textures * 2);
		for(int32_t t = 0; t < n_textures; ++t)
		{
			if(!textures[t].rgb) return ctx_fail(c, ADYPT_E_INVALID, who + "bad texture " + std::to_string(t) + ": rgb is null");
			wh[2 * t] = textures[t].width; wh[2 * t + 1] = textures[t].height;
		}
		desc.resize((size_t)n_textures * kTexDescWords);
		if(const char *why = appearance_describe(wh.data(), n_textures, desc.data(), &arena_words)) return ctx_fail(c, ADYPT_E_INVALID, who + why);
		for(int32_t t = 0; t < n_textures; ++t) plan.add(textures[t].rgb, textures[t].width, textures[t].height, (uint32_t)desc[t * kTexDescWords]);
	}
	const uint32_t tiles = plan.close();
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_STEP(ctx_drain(c));
	const CtxAppearance old = ctx_appearance(c);
	const int32_t n_tex = keep ? old.n_textures : n_textures;
	const int32_t *use_desc = keep ? old.tex_desc : desc.data();
	// the table, by the definition's words
	std::vector<uint32_t> table((size_t)std::max<int64_t>(n_mats, 1) * kMatRecordWords, 0u);
	for(int64_t m = 0; m < n_mats; ++m)
	{
		uint32_t src[kMatSourceWords];
		memcpy(src, (const uint8_t *)materials + (size_t)m * kMatSourceBytes, sizeof(src));
		for(int k = 0; k < kMatRecordWords; ++k) table[(size_t)m * kMatRecordWords + k] = material_record_word(src, k, n_tex, use_desc);
	}
	// everything that needs memory, before anything is written
	Appearance *a = ctx_state<Appearance>(c, kAttachAppearance);
	Buffer<float4> new_table;
	Buffer<uint32_t> new_arena;
	CTX_TRY(c, at_least(new_table, table.size() / 4));
	if(!keep) CTX_TRY(c, at_least(new_arena, (size_t)arena_words));
	CTX_STEP(reserve_texels(c, *a, plan));
	CTX_TRY(c, at_least(a->changed, 1));
	a->timer.invalidate();
	CTX_STEP(pack_texels(c, *a, plan, tiles, new_arena.get(), i.stream));
	CTX_TRY(c, hipMemcpyAsync(new_table.get(), table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream)); // (`table` may go; the new arrays are complete: a failure up to here has left the context as it was)
	CTX_STEP(write_attributes(c, *a, 0, ctx_scene(c).n_tris, nullptr, nullptr, new_table.get(), n_mats, n_tex, i.stream));
	ctx_replace_appearance(c, &new_table, n_mats, keep ? nullptr : &new_arena, &desc, arena_words);
	return finish(c, *a, i.stream, true); // (the old table and arena go with `new_table` and `new_arena`, the stream having been waited for)
}

int adypt_update_texture(adypt_ctx *c, int32_t index, const uint8_t *rgb, int32_t width, int32_t height)
{
	if(!c) return ADYPT_E_INVALID;
	const std::string who = "adypt_update_texture: ";
	if(!rgb) return ctx_fail(c, ADYPT_E_INVALID, who + "rgb is null");
	const CtxAppearance ap = ctx_appearance(c);
	if(index < 0 || index >= ap.n_textures) return ctx_fail(c, ADYPT_E_INVALID, who + "no texture " + std::to_string(index));
	const int32_t *d = ap.tex_desc + (size_t)index * kTexDescWords;
	if(width != d[1] || height != d[2])
		return ctx_fail(c, ADYPT_E_INVALID, who + "texture " + std::to_string(index) + " is " + std::to_string(d[1]) + " x " + std::to_string(d[2]) + " (another size: adypt_set_materials)");
	TexelPlan plan;
	plan.add(rgb, width, height, (uint32_t)d[0]);
	const uint32_t tiles = plan.close();
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_STEP(ctx_drain(c));
	Appearance *a = ctx_state<Appearance>(c, kAttachAppearance);
	CTX_STEP(reserve_texels(c, *a, plan));
	a->timer.invalidate();
	CTX_STEP(pack_texels(c, *a, plan, tiles, ctx_appearance(c).texels, i.stream));
	CTX_TRY(c, a->timer.mark(3, i.stream));
	return finish(c, *a, i.stream, false);
}

int adypt_set_triangle_attributes(adypt_ctx *c, int64_t first, int64_t count, const int32_t *material_ids, const float *texcoords)
{
	if(!c) return ADYPT_E_INVALID;
	const std::string who = "adypt_set_triangle_attributes: ";
	if(!material_ids && !texcoords) return ctx_fail(c, ADYPT_E_INVALID, who + "material_ids and texcoords are both null");
	const int64_t n = ctx_scene(c).n_tris;
	if(first < 0 || count < 0 || first > n || count > n - first) return ctx_fail(c, ADYPT_E_INVALID, who + "the range is not inside the context's triangles");
	if(!layouts_fit(c)) return ctx_fail(c, ADYPT_E_HIP, who + "the record layouts are not appearance.hpp's");
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_STEP(ctx_drain(c));
	Appearance *a = ctx_state<Appearance>(c, kAttachAppearance);
	if(material_ids) CTX_TRY(c, at_least(a->ids, (size_t)count));
	if(texcoords) CTX_TRY(c, at_least(a->texcoords, (size_t)count * 3));
	CTX_TRY(c, at_least(a->changed, 1));
	a->timer.invalidate();
	CTX_TRY(c, a->timer.mark(0, i.stream));
	if(material_ids && count) CTX_TRY(c, hipMemcpyAsync(a->ids.get(), material_ids, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, i.stream));
	if(texcoords && count) CTX_TRY(c, hipMemcpyAsync(a->texcoords.get(), texcoords, (size_t)count * kTriTexcoordWords * sizeof(float), hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, a->timer.mark(1, i.stream));
	CTX_TRY(c, a->timer.mark(2, i.stream)); // (no texels are packed)
	const CtxAppearance ap = ctx_appearance(c);
	CTX_STEP(write_attributes(c, *a, first, count, material_ids ? a->ids.get() : nullptr, texcoords ? a->texcoords.get() : nullptr, ap.materials, ap.n_mats, ap.n_textures, i.stream));
	return finish(c, *a, i.stream, true);
}

int adypt_read_material_records(adypt_ctx *c, void *out)
{
	if(!c) return ADYPT_E_INVALID;
	if(!out) return ctx_fail(c, ADYPT_E_INVALID, "adypt_read_material_records: out is null");
	const CtxInfo i = ctx_info(c);
	const CtxAppearance ap = ctx_appearance(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	if(ap.n_mats) CTX_TRY(c, hipMemcpy(out, ap.materials, (size_t)ap.n_mats * ap.mat_float4 * sizeof(float4), hipMemcpyDeviceToHost));
	return ADYPT_OK;
}

int adypt_read_texels(adypt_ctx *c, uint32_t *out)
{
	if(!c) return ADYPT_E_INVALID;
	if(!out) return ctx_fail(c, ADYPT_E_INVALID, "adypt_read_texels: out is null");
	const CtxInfo i = ctx_info(c);
	const CtxAppearance ap = ctx_appearance(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	if(ap.n_texels) CTX_TRY(c, hipMemcpy(out, ap.texels, (size_t)ap.n_texels * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return ADYPT_OK;
}

int adypt_get_appearance(adypt_ctx *c, adypt_appearance_info *out)
{
	if(!c) return ADYPT_E_INVALID;
	if(!out) return ctx_fail(c, ADYPT_E_INVALID, "adypt_get_appearance: out is null");
	const CtxAppearance ap = ctx_appearance(c);
	const Appearance *a = ctx_state_if_any<Appearance>(c, kAttachAppearance);
	*out = adypt_appearance_info{};
	out->n_mats = ap.n_mats; out->n_texels = ap.n_texels; out->n_textures = ap.n_textures;
	out->device_bytes = (int64_t)(ap.device_bytes + (a ? a->device_bytes() : 0));
	if(a && a->timer.completed())
	{
		float ms[kAppearanceStages] = {0.0f, 0.0f, 0.0f};
		(void)hipSetDevice(ctx_info(c).device);
		(void)a->timer.read(ms, kAppearanceStages, kAppearanceStages, false);
		out->reclassed = a->reclassed; out->staged_ms = ms[0]; out->packed_ms = ms[1]; out->classified_ms = ms[2];
	}
	return ADYPT_OK;
}

// the scene is replicated: the same table, texels and attributes on every device
int adypt_multi_set_materials(adypt_multi *m, const void *materials, int64_t n_mats, const adypt_texture *textures, int32_t n_textures)
{
	// (bad arguments are refused by the first context: none has changed)
	return multi_each(m, [=](adypt_ctx *c) { return adypt_set_materials(c, materials, n_mats, textures, n_textures); });
}

int adypt_multi_update_texture(adypt_multi *m, int32_t index, const uint8_t *rgb, int32_t width, int32_t height)
{
	return multi_each(m, [=](adypt_ctx *c) { return adypt_update_texture(c, index, rgb, width, height); });
}

int adypt_multi_set_triangle_attributes(adypt_multi *m, int64_t first, int64_t count, const int32_t *material_ids, const float *texcoords)
{
	return multi_each(m, [=](adypt_ctx *c) { return adypt_set_triangle_attributes(c, first, count, material_ids, texcoords); });
}

}  // extern "C"
