// Internal seam between tracer.hip (owner of struct adypt_ctx) and the other translation units of the library — multi.hip (RCCL gather of the tile
// shards), denoise.hip, refit.hip, build.hip: the few fields and functions each of them needs, without exposing the context's layout.  What those
// units are written with on top of it: ctx_unit.hpp.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include "noise.hpp"
#include "resources.hpp"
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

struct adypt_ctx;
struct adypt_multi;

namespace adypt {

struct CtxInfo {
	int device;
	hipStream_t stream;            // the context's own (non-blocking) stream: collectives are enqueued behind the rendering
	int rank, nranks, width, height;
	int n_local_px;                // owned blocks x 1024
	float4 *accum;                 // compact block-major running mean (image 0) of the owned blocks
};

CtxInfo ctx_info(adypt_ctx *c);
void ctx_set_error(adypt_ctx *c, const std::string &msg);
// What another translation unit parks in a context, which owns it from then on: released through free_fn when something else takes its place and
// by adypt_destroy (streams drained, the context's device current), the communicator first.
struct Attachment {
	void *p = nullptr;
	void (*free_fn)(void *) = nullptr;
	Attachment() = default;
	Attachment(const Attachment &) = delete;
	Attachment &operator=(const Attachment &) = delete;
	~Attachment() { reset(); }
	void reset(void *q = nullptr, void (*f)(void *) = nullptr) { if(p && free_fn) free_fn(p); p = q; free_fn = f; }
};
enum AttachKind { kAttachComm = 0, kAttachDenoise, kAttachRefit, kAttachBuild, kAttachGeometry, kAttachPose, kAttachMesh, kAttachAppearance, kAttachHistoryPlan, kAttachKinds }; // multi.hip's communicator, denoise.hip's images, refit.hip's plan and boxes, build.hip's scratch, geometry.hip's staging, pose.hip's rest pose and binding, mesh.hip's index buffer and incidence lists, appearance.hip's staging, history_plan.hip's reach image, bins and last plan
Attachment &ctx_attachment(adypt_ctx *c, AttachKind kind);

// ---- noise statistics and adaptive sampling, per context (adypt_trace_adaptive and adypt_multi_trace_adaptive are one loop over these) ----
// ADYPT_OK when the statistics are on and the image has min_spp frames, else ADYPT_E_STATE with `fn` named in the context's error
int noise_ready(adypt_ctx *c, const char *fn, int min_spp);
// noise_ready(c, fn, 0), and no look-ahead: parked frames belong to a block set that a check may change
int ctx_adaptive_ready(adypt_ctx *c, const char *fn);
// ctx_adaptive_ready, and what a plan made before the first sample of a pose needs beside it (history_plan.hip): a camera, the ray queues, a frame
// counter at 0 and no frozen block; ADYPT_E_STATE with `fn` named otherwise.  Nothing changes.
int ctx_plan_ready(adypt_ctx *c, const char *fn);
// the frame counter (adypt_get_spp)
int ctx_spp(adypt_ctx *c);
// THE reader of a context's block results (k_noise_blocks behind the frames; adypt_get_noise and adypt_read_block_noise are written on it): APPENDS
// the owned blocks, ascending, each at its own sample count; nothing for a shard that owns no block.  The caller has asked noise_ready(c, fn, 2).
int ctx_read_blocks(adypt_ctx *c, std::vector<BlockState> *blocks);
// the owned blocks among the image blocks given stop at `spp` frames
int ctx_freeze_blocks(adypt_ctx *c, const int32_t *blocks, size_t n, int spp);

// ---- the denoiser (denoise.hip), per context ----
// what ctx_denoise_inputs gives: the block-major local images the filter reads and every owned block's sample count
struct DenoiseInputs {
	const float4 *accum;               // running mean per local pixel
	const float2 *moments;             // luminance (mean, m2) per local pixel
	const int32_t *blocks;             // device: image block index of every owned block
	int n_blocks;
	std::vector<int32_t> block_index;  // host copy of `blocks`
	std::vector<int32_t> block_spp;    // samples in every owned block
};
// ADYPT_OK, or ADYPT_E_STATE with the reason in the context's error (statistics off, a viewer's image, a block below min_spp: 1 for a moments call,
// whose S0 is defined from one sample, 2 for every other)
int ctx_denoise_ready(adypt_ctx *c, const char *fn, int min_spp);
DenoiseInputs ctx_denoise_inputs(adypt_ctx *c);
// see tracer.hip
int ctx_capture_guides(adypt_ctx *c, const char *fn, float4 *albedo, float4 *normal, float4 *position, float4 *hits);
// what adypt_set_camera was last given (the guides above are captured under it): the temporal merge keeps it beside the history it commits
struct CtxCamera { float origin[3], inv_proj[16], inv_view[16]; };
CtxCamera ctx_camera(adypt_ctx *c);
// The context's own ray queues and its traversal, for the chain through mirrors and glass (guide_chain.hpp): the denoiser's kernels write the rays of a
// round into a queue, the context's k_trace finds their closest hits.  Slots: segment s owns [s * seg_cap, (s + 1) * seg_cap); a ray is (origin, tmin)
// in o[parity] and (direction, a word carried along) in d[parity]; its hit (bits(tri), u, v, t) comes in `hit` at the same slot.  The rays of segment
// s of round r are counted in count[r * round_stride + s * seg_stride], zero when ctx_ray_queues returns.
struct CtxRayQueues {
	float4 *o[2], *d[2], *hit;
	uint32_t *count;
	int rounds;                    // rounds the counters hold
	uint32_t round_stride, seg_stride;
	int segments;
	uint32_t seg_cap;              // >= ceil(owned blocks x 4 / segments) x 256: a workgroup of 256 local pixels per segment in turn always fits
	float tmin;                    // the ray_tmin of the context's parameters
};
// see tracer.hip
int ctx_ray_queues(adypt_ctx *c, const char *fn, CtxRayQueues *q);
int ctx_trace_queue(adypt_ctx *c, int parity, int round);

// ---- moving geometry (refit.hip), per context ----
// the scene arrays on the device, which refit.hip rewrites in place between frames
struct CtxScene {
	uint4 *nodes;                 // n_nodes x 80 bytes
	float4 *woop;                 // n_refs x 3
	float4 *triangles;            // n_tris records of tri_float4 float4: floats 0..8 the positions, 9..17 the normals (shade.hpp)
	const int32_t *tri_indices;   // n_refs
	int64_t n_nodes, n_refs, n_tris;
	int tri_float4;
};
CtxScene ctx_scene(adypt_ctx *c);
// the per-reference copy of the triangle records made again from the records as they are now, on the context's stream; nothing when the context keeps none
int ctx_expand_references(adypt_ctx *c);
// the root card (root_card.hpp) written again from node 0 as it is now, on the context's stream and without a host sync: behind every launch that rewrites node 0
int ctx_refresh_root_card(adypt_ctx *c);
// everything the context has enqueued on any of its streams has finished (the scene arrays are about to change under it)
int ctx_drain(adypt_ctx *c);
// ---- rebuilding the tree (build.hip), per context: see tracer.hip ----
int ctx_replace_bvh(adypt_ctx *c, Buffer<uint4> *nodes, Buffer<int32_t> *tri_indices, Buffer<float4> *woop, int64_t n_nodes, int64_t n_refs);
// ---- replacing the triangles (geometry.hip), per context: see tracer.hip ----
// what k_pack_triangles reads of a context, and whether the context keeps a class byte per triangle (ADYPT_SHADE_BIN=1)
struct CtxMaterials {
	const float4 *materials;      // n_mats records of mat_float4 float4, each beginning with the reference's 64 bytes
	int64_t n_mats;
	int n_textures, mat_float4;
	bool keeps_classes;
	const uint32_t *texels;       // the textures' texels, as the shading reads them (texture.hpp)
};
CtxMaterials ctx_materials(adypt_ctx *c);
// new triangles, packed and complete on the context's stream: taken by the context together with the tree built of them
struct NewGeometry {
	Buffer<float4> *records;      // n_tris records
	Buffer<uint8_t> *classes;     // n_tris bytes; read only where the context keeps them
	int64_t n_tris;
};
// ctx_replace_bvh that takes the triangles the tree was built of as well: records, class bytes, tree, per-reference copy and the triangle count change
// together or not at all
int ctx_replace_geometry(adypt_ctx *c, NewGeometry *geometry, Buffer<uint4> *nodes, Buffer<int32_t> *tri_indices, Buffer<float4> *woop, int64_t n_nodes, int64_t n_refs);
// ---- changing what the surfaces look like (appearance.hip), per context: see tracer.hip ----
// what appearance.hip rewrites in place or reads out: the arrays as they are now
struct CtxAppearance {
	float4 *materials;            // n_mats records of mat_float4 float4
	uint32_t *texels;             // n_texels words (appearance.hpp)
	uint8_t *tri_class;           // n_tris bytes, or null where the context keeps none
	float4 *ref_triangles;        // n_refs records, or null where the context keeps no per-reference copy
	const int32_t *tex_desc;      // HOST: n_textures descriptors (offset, w, h, 0)
	int64_t n_mats, n_texels;
	int n_textures, mat_float4;
	size_t device_bytes;          // of the table and the arena
	bool expand_whole;            // ADYPT_APPEARANCE_EXPAND=1 (measurement): the whole per-reference copy is made again, not k_ref_attributes' part of it
};
CtxAppearance ctx_appearance(adypt_ctx *c);
// The material table, and with `texels` the texture arena and its descriptors, replaced by new ones that are complete on the context's stream: table,
// arena, n_mats and n_tex change in one step, which cannot fail; the old arrays go back with the caller's owners.  texels null: the textures stay.
void ctx_replace_appearance(adypt_ctx *c, Buffer<float4> *materials, int64_t n_mats, Buffer<uint32_t> *texels, std::vector<int32_t> *tex_desc, int64_t n_texels);
// the reason adypt_last_error(NULL) gives on this thread: of a create that returned no context
void ctx_set_create_error(const std::string &msg);
// multi.hip: the message adypt_multi_last_error answers
void multi_set_error(adypt_multi *m, const std::string &msg);
// multi.hip: the reason adypt_multi_last_error(NULL) gives on this thread: of a create that returned no handle
void multi_set_create_error(const std::string &msg);
// multi.hip: the same call on every context, in device order.  The first result that is not ADYPT_OK ends it and is returned, that context's error
// becoming the handle's; ADYPT_E_INVALID for a null or empty handle.
int multi_each(adypt_multi *m, const std::function<int(adypt_ctx *)> &f);

}  // namespace adypt
