// Replacing the triangles of a context on the device (include/adypt_hip.h adypt_set_triangles, adypt_create_from_triangles; the record: tri_record.hpp).
// A translation unit of its own: nothing here is part of the tracer's code object.  What one adypt_set_triangles runs, all on the context's stream
// after the context has been drained:
//     the staging copy    the caller's n x 100 bytes as they are, into a buffer that is kept at its largest
//     k_pack_triangles    100-byte Triangle -> 128-byte record (+ the class byte where the context keeps one), into NEW arrays.  A source triangle is only
//                         4-byte aligned and a lane's 100 bytes are not a lane's 128, so the data goes through LDS: a workgroup takes 256 triangles, whose
//                         25 600 source bytes are contiguous and begin on a 16-byte boundary (256 x 100 = 1600 x 16); it reads them with 16-byte loads,
//                         neighbouring lanes neighbouring 16 bytes, looks one material up per triangle, and writes the records 16 bytes per lane, again
//                         neighbouring lanes neighbouring 16 bytes (eight lanes per record).  No lane ever walks memory at a 100- or 128-byte stride.
//     (build.hip)         the rebuild of adypt_rebuild_bvh*, reading the new records; at its end the context takes records, class bytes, tree,
//                         per-reference copy and count in one step (ctx_replace_geometry), so a refused or failed call leaves the old scene traceable.
#include "ctx_unit.hpp"
#include "build_internal.hpp"
#include "mesh_internal.hpp"
#include "pose_internal.hpp"
#include "denoise_internal.hpp"
#include "tri_record.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace adypt;

namespace {

constexpr int kPackThreads = 256;                                          // = triangles per workgroup
constexpr int kPackSourceVecs = kPackThreads * kTriSourceBytes / 16;       // 1600 x 16 bytes of source per workgroup
constexpr int kRecordVecs = kTriRecordWords / 4;                           // 8 x 16 bytes per record
constexpr int64_t kMaxTriangles = (int64_t)1 << 30;
enum PackFlag : uint32_t { kFlagNanVertex = 1u };
static_assert(kPackThreads * kTriSourceBytes % 16 == 0, "a workgroup's source bytes begin on a 16-byte boundary");
static_assert(sizeof(uint4) * kRecordVecs == 128, "the record is one 128-byte line");

// src: the staged source, 16-byte aligned, n_src_vecs = ceil(n * 100 / 16) readable uint4; records: n x 8 uint4; classes: n bytes or null; flags: one
// word, cleared by the caller, in which PackFlag bits are raised
__global__ __launch_bounds__(kPackThreads) void k_pack_triangles(const uint4 *src, int64_t n, int64_t n_src_vecs, const uint32_t *materials, int mat_words, int64_t n_mats, int n_textures,
                                                                  uint4 *records, uint8_t *classes, uint32_t *flags)
{
	__shared__ uint4 s_src[kPackSourceVecs];
	__shared__ uint32_t s_class_word[kPackThreads];
	const int tid = (int)threadIdx.x;
	const int64_t first = (int64_t)blockIdx.x * kPackThreads, vec0 = (int64_t)blockIdx.x * kPackSourceVecs;
	const int count = (int)(n - first < kPackThreads ? n - first : kPackThreads);
	for(int i = tid; i < kPackSourceVecs; i += kPackThreads)
		if(vec0 + i < n_src_vecs) s_src[i] = src[vec0 + i];
	__syncthreads();
	const uint32_t *words = (const uint32_t *)s_src;
	if(tid < count)
	{
		const int32_t matid = (int32_t)words[tid * kTriSourceWords + 24];
		const bool known = matid >= 0 && matid < n_mats;
		const TriMaterialWords w = tri_material_words(matid, n_mats, n_textures, materials + (known ? (size_t)matid * mat_words : 0));
		s_class_word[tid] = w.class_word;
		if(classes) classes[first + tid] = w.class_byte;
		// a NaN coordinate: the builders' min and max would drop it and bound the triangle as if the vertex were not there
		bool nan = false;
		for(int k = 0; k < 9; ++k) nan |= (words[tid * kTriSourceWords + k] & 0x7fffffffu) > 0x7f800000u;
		if(nan) atomicOr(flags, kFlagNanVertex);
	}
	__syncthreads();
	for(int k = 0; k < kRecordVecs; ++k)
	{
		const int o = k * kPackThreads + tid, r = o / kRecordVecs, q = o % kRecordVecs;
		if(r >= count) continue;
		const uint32_t *s = words + r * kTriSourceWords;
		const uint32_t cw = s_class_word[r];
		uint4 v;
		v.x = tri_record_word(s, q * 4, cw); v.y = tri_record_word(s, q * 4 + 1, cw); v.z = tri_record_word(s, q * 4 + 2, cw); v.w = tri_record_word(s, q * 4 + 3, cw);
		records[first * kRecordVecs + o] = v;
	}
}

constexpr int kTimingEvents = 3; // start, staged, packed

// kept per context: the staging buffer, at its largest, and the times of the last call
struct Geometry {
	Buffer<uint4> stage;
	Buffer<uint32_t> flags;
	StageTimer<kTimingEvents> timer;
};

// what adypt_set_triangles refuses before it touches the device: the reason, or empty
std::string refused(const char *who, const void *triangles, int64_t n_tris, const BuildRequest &q)
{
	const std::string w = std::string(who) + ": ";
	if(!triangles) return w + "triangles is null";
	if(n_tris < 1 || n_tris > kMaxTriangles) return w + "the number of triangles must be in [1, 2^30]";
	if(const char *why = request_refused(q)) return w + why;
	return std::string();
}

int set_triangles(adypt_ctx *c, const char *who, const void *triangles, int64_t n_tris, const BuildRequest &q, adypt_rebuild_info *out)
{
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_STEP(ctx_drain(c));
	const CtxScene sc = ctx_scene(c);
	const CtxMaterials mt = ctx_materials(c);
	if(sc.tri_float4 != kRecordVecs || mt.mat_float4 * 4 < kMatSourceWords) return ctx_fail(c, ADYPT_E_HIP, std::string(who) + ": the record layouts are not tri_record.hpp's");
	Geometry *g = ctx_state<Geometry>(c, kAttachGeometry);
	const size_t src_bytes = (size_t)n_tris * kTriSourceBytes, n_src_vecs = (src_bytes + 15) / 16;
	CTX_TRY(c, at_least(g->stage, n_src_vecs)); CTX_TRY(c, at_least(g->flags, 1));
	Buffer<float4> records;
	Buffer<uint8_t> classes;
	CTX_TRY(c, at_least(records, (size_t)n_tris * kRecordVecs));
	if(mt.keeps_classes) CTX_TRY(c, at_least(classes, (size_t)n_tris));
	g->timer.invalidate();
	CTX_TRY(c, g->timer.mark(0, i.stream));
	CTX_TRY(c, hipMemcpyAsync(g->stage.get(), triangles, src_bytes, hipMemcpyHostToDevice, i.stream));
	CTX_TRY(c, hipMemsetAsync(g->flags.get(), 0, sizeof(uint32_t), i.stream));
	CTX_TRY(c, g->timer.mark(1, i.stream));
	hipLaunchKernelGGL(k_pack_triangles, dim3(grid_of(n_tris, kPackThreads)), dim3(kPackThreads), 0, i.stream, (const uint4 *)g->stage.get(), n_tris, (int64_t)n_src_vecs,
	                   (const uint32_t *)mt.materials, mt.mat_float4 * 4, mt.n_mats, mt.n_textures, (uint4 *)records.get(), mt.keeps_classes ? classes.get() : nullptr, g->flags.get());
	CTX_TRY(c, hipGetLastError());
	CTX_TRY(c, g->timer.mark(2, i.stream));
	uint32_t flags = 0;
	CTX_TRY(c, hipMemcpyAsync(&flags, g->flags.get(), sizeof(flags), hipMemcpyDeviceToHost, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	if(flags & kFlagNanVertex) return ctx_fail(c, ADYPT_E_INVALID, std::string(who) + ": a vertex has a NaN coordinate (its triangle could never be hit, and the builders would bound it as if the vertex were not there)");
	NewGeometry geometry{&records, &classes, n_tris};
	CTX_STEP(build_for_triangles(c, q, who, (const float4 *)records.get(), &geometry, out));
	g->timer.complete(); // (the build has waited for the stream)
	pose_drop_binding(c); // (a rest pose and a binding were the old triangles': pose.hip)
	mesh_drop_binding(c); // (and so were an index buffer and its incidence lists: mesh.hip)
	denoise_triangles_replaced(c); // (and so was what the temporal merge followed moved geometry by: denoise.hip)
	return ADYPT_OK; // (the old records and class bytes go with `records` and `classes`)
}

// the description adypt_create is given before the first tree exists: one node without children and the first triangle — replaced before anyone sees it
struct Placeholder {
	uint32_t node[20] = {0};
	int32_t no_reference = 0;
	adypt_scene_desc desc;
	explicit Placeholder(const adypt_scene_desc &d) : desc(d)
	{
		desc.nodes = node; desc.n_nodes = 1; desc.tri_indices = &no_reference; desc.n_refs = 0; desc.woop = nullptr; desc.n_tris = 1;
	}
};

std::string refused_description(const char *who, const adypt_scene_desc *d)
{
	if(d->nodes || d->tri_indices || d->woop || d->n_nodes != 0 || d->n_refs != 0) return std::string(who) + ": the description names a tree (nodes, tri_indices, woop must be NULL, n_nodes and n_refs 0)";
	return std::string();
}

}  // namespace

extern "C" {

int adypt_set_triangles(adypt_ctx *c, const void *triangles, int64_t n_tris, const adypt_bvh_params *params, int method, int radius, double split_budget, adypt_rebuild_info *out)
{
	if(!c) return ADYPT_E_INVALID;
	const BuildRequest q{build_cfg(params), method, radius, split_budget};
	const std::string why = refused("adypt_set_triangles", triangles, n_tris, q);
	if(!why.empty()) return ctx_fail(c, ADYPT_E_INVALID, why);
	return set_triangles(c, "adypt_set_triangles", triangles, n_tris, q, out);
}

int64_t adypt_get_triangle_count(adypt_ctx *c) { return c ? ctx_scene(c).n_tris : (int64_t)ADYPT_E_INVALID; }

int adypt_read_triangle_records(adypt_ctx *c, void *out)
{
	if(!c || !out) return ADYPT_E_INVALID;
	const CtxScene sc = ctx_scene(c);
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	CTX_TRY(c, hipMemcpy(out, sc.triangles, (size_t)sc.n_tris * sc.tri_float4 * sizeof(float4), hipMemcpyDeviceToHost));
	return ADYPT_OK;
}

int adypt_get_set_triangles_timing(adypt_ctx *c, float *ms, int capacity)
{
	if(!c || !ms || capacity < 0) return ADYPT_E_INVALID;
	const Geometry *g = ctx_state_if_any<Geometry>(c, kAttachGeometry);
	if(!g || !g->timer.completed()) return ctx_fail(c, ADYPT_E_STATE, "adypt_get_set_triangles_timing: no triangles have been set yet (adypt_set_triangles)");
	return g->timer.read(ms, capacity, kTimingEvents - 1, true);
}

int adypt_create_from_triangles(adypt_ctx **out, const adypt_scene_desc *desc, const adypt_bvh_params *params, int method, int radius, double split_budget, adypt_rebuild_info *info)
{
	const char *who = "adypt_create_from_triangles";
	ctx_set_create_error("");
	if(!out || !desc) { ctx_set_create_error(std::string(who) + ": null argument"); return ADYPT_E_INVALID; }
	*out = nullptr;
	const BuildRequest q{build_cfg(params), method, radius, split_budget};
	std::string why = refused_description(who, desc);
	if(why.empty()) why = refused(who, desc->triangles, desc->n_tris, q);
	if(!why.empty()) { ctx_set_create_error(why); return ADYPT_E_INVALID; }
	const Placeholder first(*desc);
	adypt_ctx *c = nullptr;
	const int made = adypt_create(&c, &first.desc);
	if(made != ADYPT_OK) return made; // (the reason is adypt_create's)
	const int r = set_triangles(c, who, desc->triangles, desc->n_tris, q, info);
	if(r != ADYPT_OK)
	{
		ctx_set_create_error(adypt_last_error(c));
		adypt_destroy(c);
		return r;
	}
	*out = c;
	return ADYPT_OK;
}

// the scene is replicated: the same triangles and the same build on every device
int adypt_multi_set_triangles(adypt_multi *m, const void *triangles, int64_t n_tris, const adypt_bvh_params *params, int method, int radius, double split_budget, adypt_rebuild_info *out)
{
	// (bad arguments and a scene that cannot be built are refused by the first context: none has changed)
	return multi_each(m, [=](adypt_ctx *c) { return adypt_set_triangles(c, triangles, n_tris, params, method, radius, split_budget, out); });
}

int adypt_create_multi_from_triangles(adypt_multi **out, const adypt_scene_desc *desc, const int *device_ids, int n_dev, const adypt_bvh_params *params, int method, int radius,
                                      double split_budget, adypt_rebuild_info *info)
{
	const char *who = "adypt_create_multi_from_triangles";
	multi_set_create_error("");
	if(!out || !desc) { multi_set_create_error(std::string(who) + ": null argument"); return ADYPT_E_INVALID; }
	*out = nullptr;
	std::string why = refused_description(who, desc);
	if(why.empty()) why = refused(who, desc->triangles, desc->n_tris, BuildRequest{build_cfg(params), method, radius, split_budget});
	if(!why.empty()) { multi_set_create_error(why); return ADYPT_E_INVALID; }
	const Placeholder first(*desc);
	adypt_multi *m = nullptr;
	const int made = adypt_create_multi(&m, &first.desc, device_ids, n_dev);
	if(made != ADYPT_OK) return made; // (the reason is adypt_create_multi's)
	const int r = adypt_multi_set_triangles(m, desc->triangles, desc->n_tris, params, method, radius, split_budget, info);
	if(r != ADYPT_OK)
	{
		multi_set_create_error(adypt_multi_last_error(m));
		adypt_destroy_multi(m);
		return r;
	}
	*out = m;
	return ADYPT_OK;
}

}  // extern "C"
