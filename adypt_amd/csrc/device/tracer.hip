// C-ABI implementation of include/adypt_hip.h: context, HBM residency of the scene, launch sequencing of the
// wavefront path tracer.  Replaces OglScene + OglPathTracer (src/Tracer/*.cpp) of the reference.
//
// Per frame (= one OglPathTracer::Trace(true), OglPathTracer.cpp:34-61):
//     memset counters -> k_gen_primary -> [ k_trace -> k_shade ] x maxBounce      (no host sync; queue sizes live in
//     device memory, the traversal kernel is persistent, the shade grid covers the worst case)
// or, by default, k_shade_first -> k_path: the reference has no barrier between bounces at all (one dispatch runs the whole
// for(b < uMaxBounce) loop, shaders/pathtracer.glsl:107).  Which of the two a pass takes: frame_plan.hpp; how it is enqueued: frame_schedule.hpp.
// This is the ONE translation unit that instantiates the traversal / path kernels; its sections: context.hpp (struct adypt_ctx), the launch
// helpers below, scene_upload.hpp, frame_schedule.hpp, the C ABI.
// There is no CPU fallback anywhere in this file: without a HIP device adypt_create fails with ADYPT_E_NO_DEVICE.
#include "context.hpp"
#include "ctx_access.hpp"
#include "trace_until.hpp"
#include "active_blocks.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace adypt;

namespace {

thread_local std::string g_create_error;

// Zeroes the counters of `n` pipes.  A kernel rather than hipMemsetAsync: while round 3's queue corruption was being hunted (the
// append_slot fault) the memset was suspected of not being ordered against the kernels around it and replaced; that changed the timing, not the
// fault — the suspicion was never established.  The kernel stays because it is one launch for all pipes' counters and certainly stream-ordered.
__global__ void k_clear_counters(uint4 *p, uint32_t n16) { const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; if(i < n16) p[i] = make_uint4(0, 0, 0, 0); }

// Slot-claim audit (adypt_set_instrumentation flag 4).  append_slot (shade.hpp) hands every surviving path of a workgroup a slot of its queue
// segment; round 3 saw a build in which whole waves claimed ONE slot (the append_slot fault).  With the audit on, the queue a kernel is
// about to append to is filled with a poison path word, and after the kernel every slot below the segment's counter must hold a real path word, every
// path id must appear once (a bitmap over the path ids), and every slot above the counter must still be poison.
constexpr uint32_t kAuditPoison = 0xffffffffu;
__global__ void k_audit_poison(float4 *out_d, size_t n, uint32_t *seen, size_t n_seen)
{
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i < n) out_d[i].w = __uint_as_float(kAuditPoison);
	if(i < n_seen) seen[i] = 0u;
}
__global__ void k_audit_check(const float4 *out_d, const uint32_t *count, uint32_t seg_cap, uint32_t *seen, uint32_t id_limit, unsigned long long *errors)
{
	const uint32_t seg = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= seg_cap) return;
	const uint32_t w = __float_as_uint(out_d[(size_t)seg * seg_cap + i].w);
	bool bad;
	if(i < count[seg * kCursorStride])
	{
		const uint32_t id = w & kPathIdMask;
		// never written, a path id the bitmap has no bit for (a corrupted word: counted, the bitmap is not touched), or a path that holds two slots
		bad = w == kAuditPoison || id >= id_limit || ((atomicOr(&seen[id >> 5], 1u << (id & 31u)) >> (id & 31u)) & 1u);
	}
	else bad = w != kAuditPoison;                                                                     // written beyond what the counter admits
	if(bad) atomicAdd(errors, 1ull);
}

// out[r] = the 128-byte device record of triangle tri_indices[r]: the uTriIndices remap (traversal.glsl:253-254) applied to the data once, so that k_path
// looks a hit's triangle up by the traversal's own reference index.  One thread per 16 bytes.
__global__ void k_expand_references(const float4 *triangles, const int32_t *tri_indices, size_t n_refs, float4 *out)
{
	const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if(i < n_refs * kTriFloat4) out[i] = triangles[(size_t)tri_indices[i / kTriFloat4] * kTriFloat4 + i % kTriFloat4];
}

// node 0 decoded into the root card (root_card.hpp: the definition, which the host's adypt_decode_root_card compiles too).  One workgroup; the card is a few
// hundred bytes decoded once per scene change, so one lane does it and the others have nothing to add.
__global__ __launch_bounds__(64) void k_root_card(const uint4 *nodes, int allow, RootCard *card)
{
	if(threadIdx.x != 0 || blockIdx.x != 0) return;
	uint32_t n[20];
	for(int i = 0; i < kNodeUint4; ++i) { const uint4 v = nodes[i]; n[4 * i] = v.x; n[4 * i + 1] = v.y; n[4 * i + 2] = v.z; n[4 * i + 3] = v.w; }
	RootCard rc;
	decode_root_card(n, allow != 0, &rc);
	*card = rc;
}

template <class D, class T> int upload(adypt_ctx *c, Buffer<D> *dst, const T *src, size_t n)
{
	HIP_TRY(c, dst->alloc(std::max<size_t>(n * sizeof(T), 16)));
	if(n) HIP_TRY(c, hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
	return ADYPT_OK;
}

// `b` holds at least `bytes` afterwards.  Before the old array goes, what may still be using it is drained: the context's stream, or the whole
// device where launches of any pipe may.  What the array held is not kept.
template <class T> int grow(adypt_ctx *c, Buffer<T> &b, size_t bytes, bool whole_device = false)
{
	if(b.bytes() >= bytes) return ADYPT_OK;
	HIP_TRY(c, whole_device ? hipDeviceSynchronize() : hipStreamSynchronize(c->stream));
	HIP_TRY(c, b.alloc(bytes));
	return ADYPT_OK;
}

// The two run-time flags of a traversal launch as compile-time ones: f(std::bool_constant<a>, std::bool_constant<b>), so that a launcher
// names its kernel template once.  (The order of the arms is the order in which the four instances are emitted.)
template <class F> void with_flags(bool a, bool b, F &&f)
{
	if(b) { if(a) f(std::true_type{}, std::true_type{}); else f(std::false_type{}, std::true_type{}); }
	else if(a) f(std::true_type{}, std::false_type{}); else f(std::false_type{}, std::false_type{});
}

// Structural validation of the BVH arrays: a corrupt child/triangle range would make the kernel read out of
// bounds, which on this hardware can reset the GPU.  Mirrors exactly the address arithmetic of k_trace.
bool validate_bvh(const adypt_scene_desc &d, std::string *why)
{
	if(d.n_nodes <= 0) { *why = "empty node array"; return false; }
	const uint8_t *nodes = (const uint8_t *)d.nodes;
	for(int64_t i = 0; i < d.n_nodes; ++i)
	{
		const uint8_t *n = nodes + i * 80;
		uint32_t child_base, tri_base;
		memcpy(&child_base, n + 16, 4);
		memcpy(&tri_base, n + 20, 4);
		const uint8_t imask = n[15];
		const uint8_t *meta = n + 24;
		int n_inner = __builtin_popcount(imask);
		if(n_inner && (uint64_t)child_base + (uint64_t)n_inner > (uint64_t)d.n_nodes) { *why = "node " + std::to_string(i) + ": child range out of bounds"; return false; }
		for(int s = 0; s < 8; ++s)
		{
			const uint32_t m = meta[s];
			if(m == 0) continue;
			const bool inner = (m & (m << 1)) & 0x10;
			if(inner)
			{
				// hit bit (24 + widx) must address a set imask bit, and ONLY that bit may be raised: the kernel ORs
				// child_bits << bit_index into the hit mask, so child_bits other than 0b001 would mark slots that are not in
				// imask and the child index base + popcount(imask below slot) could step one past the validated range
				const uint32_t widx = (m & 31u) - 24u;
				if((m >> 5) != 1u) { *why = "node " + std::to_string(i) + ": inner child with child bits != 001"; return false; }
				if(widx > 7 || !((imask >> widx) & 1u)) { *why = "node " + std::to_string(i) + ": inner child not in imask"; return false; }
			}
			else
			{
				const uint32_t off = m & 31u, bits = (m >> 5) & 7u;
				const uint32_t top = bits ? 32u - (uint32_t)__builtin_clz(bits) : 0u;
				if(off + top > 24u) { *why = "node " + std::to_string(i) + ": leaf bits exceed 24"; return false; }
				if((uint64_t)tri_base + off + top > (uint64_t)d.n_refs) { *why = "node " + std::to_string(i) + ": triangle range out of bounds"; return false; }
			}
		}
	}
	for(int64_t i = 0; i < d.n_refs; ++i)
		if(d.tri_indices[i] < 0 || d.tri_indices[i] >= d.n_tris) { *why = "tri_indices[" + std::to_string(i) + "] out of range"; return false; }
	return true;
}

hipEvent_t begin_timing(adypt_ctx *c, int kind, hipStream_t stream)
{
	if(!(c->instrumentation & 1)) return nullptr;
	EventPair p;
	if(!c->free_events.empty()) { p = std::move(c->free_events.back()); c->free_events.pop_back(); }
	else { if(hipEventCreate(p.a.out()) != hipSuccess || hipEventCreate(p.b.out()) != hipSuccess) return nullptr; }
	p.kind = kind;
	c->events.push_back(std::move(p));
	(void)hipEventRecord(c->events.back().a, stream);
	return c->events.back().b;
}
inline void end_timing(hipEvent_t stop, hipStream_t stream) { if(stop) (void)hipEventRecord(stop, stream); }

void harvest_events(adypt_ctx *c)
{
	std::vector<EventPair> pending; // launches of a frame started ahead on its own stream may still be running: their turn comes later
	for(EventPair &p : c->events)
	{
		if(hipEventQuery(p.b) == hipErrorNotReady) { pending.push_back(std::move(p)); continue; }
		float ms = 0.0f;
		if(hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess)
		{
			if(p.kind == 0 || p.kind == 2) { c->trace_ms += ms; ++c->trace_launches; } else c->shade_ms += ms;
			if(p.kind == 2) { c->path_ms += ms; ++c->path_launches; }
		}
		c->free_events.push_back(std::move(p));
	}
	c->events.swap(pending);
}

void clear_counters(adypt_ctx *c, FrameCounters *first, int n, hipStream_t stream)
{
	static_assert(sizeof(FrameCounters) % 16 == 0, "FrameCounters is cleared 16 bytes at a time");
	const uint32_t n16 = (uint32_t)(sizeof(FrameCounters) / 16) * (uint32_t)n;
	hipLaunchKernelGGL(k_clear_counters, dim3((n16 + 255) / 256), dim3(256), 0, stream, (uint4 *)first, n16);
}

int ensure_spill(adypt_ctx *c, int stack_size)
{
	const int extra = stack_size - c->lds_depth, extra_path = c->path_blocks ? stack_size - c->path_lds_depth : 0;
	if(extra <= 0 && extra_path <= 0) return ADYPT_OK;
	const size_t per_pipe = std::max((size_t)std::max(extra, 0) * (size_t)c->trace_blocks, (size_t)std::max(extra_path, 0) * (size_t)c->path_blocks) * kTraceThreads;
	TRY_CREATE(grow(c, c->d_spill, per_pipe * kMaxPipes * sizeof(uint2), true)); // launches of any pipe may still be using the old array
	for(int k = 0; k < kMaxPipes; ++k) c->pipes[k].spill = c->d_spill + (size_t)k * per_pipe;
	return ADYPT_OK;
}

// geometry of the persistent traversal launch for a given stack size
int configure_trace(adypt_ctx *c, int stack_size)
{
	c->lds_depth = std::max(1, std::min(stack_size, kLdsStackMax));
	// testing / tuning hook: a smaller LDS part pushes stack entries into the global spill array (tests cover that path)
	if(c->tun.lds_stack_depth > 0) c->lds_depth = std::max(1, std::min(c->lds_depth, c->tun.lds_stack_depth));
	size_t lds = (size_t)(kTraceThreads / 64) * c->lds_depth * 64 * sizeof(uint2) + sizeof(WgPool) + kTripTabBytes; // stacks + the workgroup's ray pool + the waves' triangle hand-out tables
	int per_cu = 0;
	HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_trace<false>, kTraceThreads, lds));
	c->occupancy_api = per_cu;
	per_cu = std::max(1, std::min(per_cu, 8));
	// 80 VGPRs allow 6 waves per SIMD.  Measured (round 3, tools/sweep_env.py): 6 instead of 5 workgroups per CU is +2.6 % on the bench scene
	// (BVH 20 MB), +2 % on the 1.2 M-triangle scene (69 MB) and -1 % on the 10 M-triangle scene (602 MB), where the sixth wave's lines evict
	// the others' from the caches: a BVH beyond the 256 MB Infinity Cache keeps 5
	const size_t bvh_bytes = (size_t)c->n_nodes * 80 + (size_t)c->n_refs * 52;
	if(bvh_bytes > ((size_t)256 << 20)) per_cu = std::min(per_cu, 5);
	if(c->tun.trace_blocks_per_cu > 0) // tuning override
	{
		const int want = c->tun.trace_blocks_per_cu;
		// Fewer workgroups per CU than the registers allow: the traversal launches of two pipes overlap, and together they would
		// fill the CU again — so the launch asks for as much LDS as makes `want` workgroups the most that fit in a CU's 160 KB
		if(want < per_cu) lds = std::max(lds, std::min<size_t>(64 * 1024, ((c->lds_per_cu - 2048) / (size_t)want) & ~(size_t)1023));
		per_cu = want;
	}
	c->lds_bytes = lds;
	c->trace_blocks = c->num_cus * per_cu;
	// k_path (path.hpp): as many workgroups per CU as its registers allow, with the deepest LDS stack that still fits next to the path table
	{
		// (the shipped geometry — 352 slots, LDS stack depth 4 — at six workgroups per CU: 26 592 bytes, root_mask's 352 included, inside the 26 KiB the rule below gives)
		static_assert(ADYPT_PATH_SLOTS != 352 || (path_lds_bytes(4) == 26592 && path_lds_bytes(4) <= ((160 * 1024 - 2048) / 1024 / 6) * 1024), "k_path: six workgroups per CU at LDS stack depth 4");
		const int want0 = c->tun.path_blocks_per_cu > 0 ? c->tun.path_blocks_per_cu : 6;
		const size_t fixed = path_lds_bytes(0), per_entry = (size_t)(kTraceThreads / 64) * 64 * sizeof(uint2);
		int chosen = 0, depth = 1;
		for(int want = want0; want >= 1 && !chosen; --want)
		{
			// LDS is handed out in granules; the occupancy query does not know: measured, it answers 6 for 26944 bytes per workgroup, of which a
			// compute unit then runs 5 at a time (the sixth of every six waits for a slot: -5 %).  So the budget is whole KiB of (LDS per CU) / want.
			// ... of (LDS per CU - 2 KiB) / want: measured (round 6, tools/sweep_env.py), 5 workgroups of 32384 bytes = 161920 of the CU's 163840 do NOT run together — the
			// "5 per CU" of rounds 4-5 ran 4 (the rate of ADYPT_PATH_BLOCKS_PER_CU=4 to the percent) — while 5 of 30336 do
			const size_t budget = std::min<size_t>((((c->lds_per_cu - 2048) / 1024) / (size_t)want) * 1024, 64 * 1024);
			if(budget < fixed + per_entry) continue;
			int d = (int)std::min<size_t>((size_t)std::min(stack_size, kLdsStackMax), (budget - fixed) / per_entry);
			if(c->tun.path_lds_depth > 0) d = std::max(1, std::min(d, c->tun.path_lds_depth));
			int got = 0; // the query is made with THIS want's depth, and judged against this want
			HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&got, (k_path<false, false>), kTraceThreads, path_lds_bytes(d)));
			int got_sun = 0; // (the variant with sun-visibility queries among its rays must fit as well: the launch geometry is one)
			HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&got_sun, (k_path<false, true>), kTraceThreads, path_lds_bytes(d)));
			got = std::min(got, got_sun);
			if(got >= want) { chosen = want; depth = d; }
		}
		if(!chosen) return fail(c, ADYPT_E_HIP, "k_path does not fit a compute unit");
		c->path_lds_depth = depth; c->path_lds = path_lds_bytes(depth);
		c->path_blocks = c->num_cus * chosen;
		if(c->tun.path_verbose) fprintf(stderr, "[adypt] k_path: %d workgroups per CU, %d path slots each, LDS stack depth %d, %zu bytes of LDS; a hit's triangle record by %s\n", chosen, kPathSlots, depth, c->path_lds,
		                                c->d_ref_triangles ? "reference index (per-reference copy of the records)" : "uTriIndices remap in the shading round (no per-reference copy)");
	}
	return ensure_spill(c, stack_size);
}

// bounces b0 .. maxBounce-1 of a batched pass in one launch: the queue of parity `parity` holds the pass's rays of bounce b0
int launch_path(adypt_ctx *c, const Pipe &pipe, const QueueWindow &win, int parity, const uint32_t *count, uint32_t *cursor, const FrameArgs &f, const SceneArgs &sc,
				const PixelArgs &px, int b0, bool stats)
{
	PathArgs a;
	a.nodes = (const uint4 *)c->d_nodes; a.woop = (const float4 *)c->d_woop;
	a.in_o = (const float *)c->q.o[parity].get() + 3 * win.offset; a.in_d = c->q.d[parity] + win.offset; a.in_col = (const float *)c->q.col[parity].get() + 3 * win.offset;
	a.ray_stats = nullptr;
	// the triangle records by REFERENCE index when the context holds that copy, else the uTriIndices remap inside k_path
	SceneArgs sc_ref = sc;
	if(c->d_ref_triangles) sc_ref.triangles = (const float4 *)c->d_ref_triangles;
	a.tri_remap = c->d_ref_triangles ? nullptr : (const int32_t *)c->d_tri_indices;
	a.count = count; a.cursor = cursor;
	a.spill = pipe.spill; a.stats = c->d_stats;
	a.seg_cap = win.seg_cap;
	a.stack_size = c->params.stack_size; a.lds_depth = c->path_lds_depth;
	a.refill_min = c->refill_min; a.shade_min = c->shade_min; a.rare_min = c->rare_min; a.defer_max = c->defer_max;
	a.b0 = b0; a.tmin = c->params.ray_tmin;
	a.root_card = c->d_root_card;
	hipEvent_t stop = begin_timing(c, 2, pipe.stream);
	const PathKernArgs K{a, f, sc_ref, px, stats ? 1 : 0};
	// (the SUN variant: rays that end at their first accepted triangle among the others — only where the queue can hold such queries)
	with_flags(stats, f.sun_query != 0, [&](auto S, auto Sun) {
		hipLaunchKernelGGL((k_path<decltype(S)::value, decltype(Sun)::value>), dim3(c->path_blocks), dim3(kTraceThreads), c->path_lds, pipe.stream, K);
	});
	end_timing(stop, pipe.stream);
	HIP_TRY(c, hipGetLastError());
	return ADYPT_OK;
}

int launch_trace(adypt_ctx *c, const Pipe &pipe, const QueueWindow &win, int parity, const uint32_t *count, uint32_t *cursor, int stack_size, bool stats,
				 RayStats *ray_stats, bool any_hit = false, bool shadow_queue = false, bool packed = false, bool camera_rays = false)
{
	TraceArgs a;
	a.nodes = (const uint4 *)c->d_nodes;
	a.woop = (const float4 *)c->d_woop;
	a.tri_indices = (const int32_t *)c->d_tri_indices;
	// the path tracer's own queues hold 12-byte origins and hits (shade.hpp); ray batches handed in by the caller and the sun-visibility
	// queue are float4 records.  The buffers are allocated 16 bytes per slot either way; a window starts 3 (or 4) floats x offset in.
	a.packed = packed ? 1u : 0u; a.tmin = c->params.ray_tmin;
	if(packed)
	{
		a.ray_o = (const float4 *)((const float *)c->q.o[parity].get() + 3 * win.offset);
		a.hit = (float4 *)((float *)c->q.hit.get() + 3 * win.offset);
		a.ray_d = c->q.d[parity] + win.offset;
	}
	else
	{
		a.ray_o = (shadow_queue ? c->q.sh_o : c->q.o[parity]) + win.offset; a.ray_d = (shadow_queue ? c->q.sh_d : c->q.d[parity]) + win.offset;
		a.hit = (shadow_queue ? c->q.sh_hit : c->q.hit) + win.offset;
	}
	a.ray_stats = ray_stats;
	a.count = count; a.cursor = cursor;
	a.spill = pipe.spill;
	a.stats = c->d_stats;
	a.seg_cap = win.seg_cap;
	a.refill_min = camera_rays ? c->refill_min_primary : c->refill_min; a.chunk = c->chunk; a.bite = camera_rays ? c->bite_primary : c->bite; a.endgame = c->endgame;
	a.stack_size = stack_size; a.lds_depth = c->lds_depth;
	hipEvent_t stop = begin_timing(c, 0, pipe.stream);
	with_flags(stats, any_hit, [&](auto S, auto Any) {
		hipLaunchKernelGGL((k_trace<decltype(S)::value, decltype(Any)::value>), dim3(c->trace_blocks), dim3(kTraceThreads), c->lds_bytes, pipe.stream, a);
	});
	end_timing(stop, pipe.stream);
	HIP_TRY(c, hipGetLastError());
	return ADYPT_OK;
}

// the block list of a pass: the owned blocks, or the active ones among them while blocks are frozen (active_blocks.hpp)
const int32_t *pass_blocks(const adypt_ctx *c) { return c->ab.any_frozen() ? (const int32_t *)c->adaptive.blocks : (const int32_t *)c->d_local_blocks; }

void fill_frame(const adypt_ctx *c, FrameArgs *f)
{
	memset(f, 0, sizeof(*f));
	memcpy(f->inv_proj, c->inv_proj, 64); memcpy(f->inv_view, c->inv_view, 64);
	memcpy(f->origin, c->origin, 12);
	f->tmin = c->params.ray_tmin;
	memcpy(f->sun, c->params.sun, 12);
	f->clamp = c->params.clamp;
	f->width = c->width; f->height = c->height;
	f->spp = c->spp; f->subpixel = c->params.subpixel; f->tmp_life = c->params.tmp_lifetime; f->max_bounce = c->params.max_bounce;
	f->sobol = c->d_sobol; f->done = c->q.done; f->n_frames = 1; f->frame_first = 0; f->frame_stride = 1; f->batched = 0;
	f->n_local_px = c->pass_px; f->blocks_x = c->blocks_x; f->rank = c->rank; f->nranks = c->nranks;
	f->n_tris = (int32_t)c->n_tris; f->n_mats = (int32_t)c->n_mats; f->n_tex = c->n_tex;
	f->deal_chunks = c->deal_chunks;
	memcpy(f->sun_query_dir, c->sun_dir, 12); f->sun_query = 0; // (set by the frame driver where the one-launch pipeline carries the query)
}
void fill_scene(const adypt_ctx *c, SceneArgs *s)
{
	s->triangles = (const float4 *)c->d_triangles;
	s->materials = (const float4 *)c->d_materials;
	s->texels = (const uint32_t *)c->d_texels;
	s->local_blocks = pass_blocks(c);
	s->tri_class = (const uint8_t *)c->d_tri_class;
}
void fill_pixels(const adypt_ctx *c, PixelArgs *p)
{
	p->accum = c->d_accum; p->cache = c->d_cache; p->cache_next = c->d_cache_next; p->shift = c->ab.any_frozen() ? c->adaptive.shift.get() : c->d_shift.get(); p->stats = c->d_stats;
}
// slots per segment that `frames` frames of `px` pixels need (multiple of kShadeThreads)
uint32_t seg_slots_px(int px, int frames)
{
	const size_t paths = (size_t)std::max(px, 64) * (size_t)std::max(1, frames);
	const size_t chunks = (paths + kShadeThreads - 1) / kShadeThreads;
	return (uint32_t)(((chunks + kNumSegments - 1) / kNumSegments) * kShadeThreads);
}
// ... of this context's pixels: what the queues and their windows are sized by, whatever is frozen
uint32_t seg_slots_for(const adypt_ctx *c, int frames) { return seg_slots_px(c->n_local_px, frames); }
// paths per queue segment of a pass over `frames` frames (QueueArgs::seg_paths); its kernels run 8 x seg_paths / 256 workgroups.
// Sizing the grids for the allocated capacity instead cost ~6 ns per empty workgroup: 13 ms per 8-bounce batch at 66 M slots.
uint32_t pass_seg_paths(const adypt_ctx *c, const QueueWindow &win, int frames) { return std::min(win.seg_cap, seg_slots_px(c->pass_px, frames)); }

inline QueueWindow full_window(const adypt_ctx *c) { return QueueWindow{0, c->seg_cap}; }
// window of sub-batch k when a batch is cut into n_pipes sub-batches of at most ceil(frames_in_flight / n_pipes) frames
inline QueueWindow pipe_window(const adypt_ctx *c, int k, int n_pipes)
{
	if(n_pipes <= 1) return full_window(c);
	const uint32_t cap = seg_slots_for(c, (c->frames_in_flight + n_pipes - 1) / n_pipes);
	return QueueWindow{(size_t)k * (size_t)cap * kNumSegments, cap};
}

// Camera rays of a pass -> traversal -> cache images, one launch (k_trace_camera) and nothing in front of it.  `f` names the frames of the pass
// (n_frames, frame_first, frame_stride).  On the context's stream only: the launches share one set of fetch cursors.
// owned: over the OWNED blocks whatever is frozen (the denoiser's guide capture; f.n_local_px is then the owned pixels'), not over the pass's.
int launch_trace_camera(adypt_ctx *c, const Pipe &pipe, const QueueWindow &win, const FrameArgs &f, const PixelArgs &px, int bias_mode, bool stats, int viewer_type = -1, bool owned = false)
{
	TraceCameraArgs K;
	memset(&K, 0, sizeof(K));
	TraceArgs &a = K.a;
	a.nodes = (const uint4 *)c->d_nodes; a.woop = (const float4 *)c->d_woop; a.tri_indices = (const int32_t *)c->d_tri_indices;
	a.packed = 1u; a.tmin = c->params.ray_tmin;
	a.cursor = c->d_camera_cursors; K.left = c->d_camera_cursors + kNumSegments * kCursorStride;
	a.spill = pipe.spill; a.stats = c->d_stats;
	K.seg_paths = owned ? std::min(win.seg_cap, seg_slots_px(c->n_local_px, f.n_frames)) : pass_seg_paths(c, win, f.n_frames);
	K.seg_shift = 8;
	while((1u << K.seg_shift) < K.seg_paths) ++K.seg_shift;
	a.seg_cap = 1u << K.seg_shift; // (positions are numbers: nothing is stored at them)
	K.rays = (unsigned long long)(owned ? c->n_image_px : c->pass_image_px) * (unsigned long long)f.n_frames;
	a.refill_min = c->refill_min_primary; a.chunk = c->chunk; a.bite = c->bite_primary; a.endgame = c->endgame;
	a.stack_size = c->params.stack_size; a.lds_depth = c->lds_depth;
	K.f = f; K.local_blocks = owned ? (const int32_t *)c->d_local_blocks : pass_blocks(c); K.px = px; K.bias_mode = bias_mode;
	hipEvent_t stop = begin_timing(c, 0, pipe.stream);
	const bool viewer = viewer_type >= 0; // a primary-only call: the pixel is coloured when its ray has finished (no viewer launch)
	if(viewer) { fill_scene(c, &K.sc); K.sc.local_blocks = K.local_blocks; K.viewer_type = viewer_type; }
	with_flags(stats, viewer, [&](auto S, auto Viewer) {
		hipLaunchKernelGGL((k_trace_camera<decltype(S)::value, decltype(Viewer)::value>), dim3(c->trace_blocks), dim3(kTraceThreads), c->lds_bytes, pipe.stream, K);
	});
	end_timing(stop, pipe.stream);
	HIP_TRY(c, hipGetLastError());
	return ADYPT_OK;
}

QueueArgs queue_args(adypt_ctx *c, const QueueWindow &win, int in, const uint32_t *count_in, uint32_t *count_out, int frames = 0)
{
	QueueArgs q;
	q.seg_paths = frames > 0 ? pass_seg_paths(c, win, frames) : win.seg_cap;
	q.ray_o = (float *)c->q.o[in].get() + 3 * win.offset; q.ray_d = c->q.d[in] + win.offset; q.col = (float *)c->q.col[in].get() + 3 * win.offset;
	q.hit = (float *)c->q.hit.get() + 3 * win.offset;
	q.out_o = (float *)c->q.o[in ^ 1].get() + 3 * win.offset; q.out_d = c->q.d[in ^ 1] + win.offset; q.out_col = (float *)c->q.col[in ^ 1].get() + 3 * win.offset;
	q.count_in = count_in; q.count_out = count_out;
	q.seg_cap = win.seg_cap;
	return q;
}

int check_async_errors(adypt_ctx *c)
{
	// (after a synchronisation of the streams the kernels ran on: the word is in pinned host memory, the kernels write it themselves)
	if(*(volatile uint32_t *)c->h_overflow) return fail(c, ADYPT_E_STACK_OVERFLOW, "traversal stack overflow: increase pathTracer.stackSize (currently " + std::to_string(c->params.stack_size) + ")");
	return ADYPT_OK;
}

int load_shift(adypt_ctx *c)
{
	if(c->shift_loaded && c->shift_seed_loaded == c->params.shift_seed) return ADYPT_OK;
	std::vector<uint8_t> full((size_t)c->width * c->height * 2), local((size_t)c->n_local_px * 2, 0);
	adypt_shift_bytes(c->params.shift_seed, c->width, c->height, full.data());
	for_each_local_pixel(c->local_blocks, c->width, c->height, [&](size_t L, int x, int y) {
		local[L * 2] = full[((size_t)y * c->width + x) * 2];
		local[L * 2 + 1] = full[((size_t)y * c->width + x) * 2 + 1];
	});
	// frames enqueued earlier (adypt_trace_spp_async, then adypt_reset + adypt_set_params) may still be reading d_shift
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if(!local.empty()) HIP_TRY(c, hipMemcpy(c->d_shift, local.data(), local.size(), hipMemcpyHostToDevice));
	c->shift_loaded = true; c->shift_seed_loaded = c->params.shift_seed;
	return ADYPT_OK;
}

// (re)allocate the wavefront queues for `fif` frames in flight: capacity = fif x local pixels, cut into 8 segments
int alloc_queues_raw(adypt_ctx *c, int fif)
{
	c->q = Queues{}; // the old ones go FIRST: old and new together would double the peak.  (The sun-visibility queue and the ray statistics come back when asked for)
	const size_t npx = (size_t)std::max(c->n_local_px, 64);
	const size_t paths = npx * (size_t)fif;
	if(paths >= ((size_t)1 << 31)) return fail(c, ADYPT_E_INVALID, "frames in flight x pixels exceeds 2^31 paths");
	c->seg_cap = seg_slots_for(c, fif);
	c->capacity = (int64_t)c->seg_cap * kNumSegments;
	c->frames_in_flight = fif;
	size_t nq = (size_t)c->capacity;
	for(int n = 2; n <= kMaxPipes; ++n) // the windows of an n-way split round up one by one
		nq = std::max(nq, (size_t)n * kNumSegments * (size_t)seg_slots_for(c, (fif + n - 1) / n));
	c->alloc_slots = nq;
	for(int i = 0; i < 2; ++i)
	{
		HIP_TRY(c, c->q.o[i].alloc(nq * sizeof(float4)));
		HIP_TRY(c, c->q.d[i].alloc(nq * sizeof(float4)));
		HIP_TRY(c, c->q.col[i].alloc(nq * sizeof(float4)));
	}
	HIP_TRY(c, c->q.hit.alloc(nq * sizeof(float4)));
	// finished samples of a batch / parked radiance of live paths; two frames at least: single frames in a row alternate between two slots
	HIP_TRY(c, c->q.done.alloc(npx * (size_t)std::max(fif, 2) * sizeof(float4)));
	return ADYPT_OK;
}

// A failed (re)allocation must not leave a context that launches kernels on null queues: fall back to the previous
// frames-in-flight; if even that cannot be had, the context is marked unusable and every trace call returns ADYPT_E_STATE.
int alloc_queues(adypt_ctx *c, int fif)
{
	const int previous = c->queues_ok ? c->frames_in_flight : 0;
	int r = alloc_queues_raw(c, fif);
	c->queues_ok = r == ADYPT_OK;
	if(r == ADYPT_OK) return r;
	const std::string why = c->error;
	(void)hipGetLastError();
	if(previous > 0 && previous != fif && alloc_queues_raw(c, previous) == ADYPT_OK)
	{
		c->queues_ok = true;
		c->error = why + " (kept " + std::to_string(previous) + " frames in flight)";
		return r;
	}
	// nothing usable is left: free the partial allocation of the failed attempt
	c->q = Queues{};
	c->capacity = 0; c->seg_cap = 0; c->alloc_slots = 0; c->frames_in_flight = previous;
	c->error = why + " (the context has no ray queues left: destroy it)";
	return r;
}

int ensure_shadow_queue(adypt_ctx *c)
{
	if(c->q.sh_o) return ADYPT_OK;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	const size_t nq = c->alloc_slots;
	HIP_TRY(c, c->q.sh_o.alloc(nq * sizeof(float4)));
	HIP_TRY(c, c->q.sh_d.alloc(nq * sizeof(float4)));
	HIP_TRY(c, c->q.sh_col.alloc(nq * sizeof(float4)));
	HIP_TRY(c, c->q.sh_hit.alloc(nq * sizeof(float4)));
	return ADYPT_OK;
}

// (the previous batch may still be reading the slices about to be freed; they hold nothing between batches)
int ensure_cache_slices(adypt_ctx *c, int extra) { return grow(c, c->d_cache_next, (size_t)extra * (size_t)std::max(c->n_local_px, 64) * sizeof(float4)); }

// the audit's bitmap over the path ids (one bit per queue slot is enough: ids are < capacity), one bitmap per chain: they check concurrently
int ensure_audit(adypt_ctx *c) { return grow(c, c->d_audit_seen, (((size_t)c->alloc_slots + 31) / 32 + 1) * kMaxPipes * sizeof(uint32_t), true); }
size_t audit_words(const adypt_ctx *c) { return c->d_audit_seen.bytes() / (kMaxPipes * sizeof(uint32_t)); } // words of ONE bitmap
// around a kernel that appends to q's output queue: poison before, check after (both on the launch's stream)
void audit_before(adypt_ctx *c, const QueueArgs &q, hipStream_t stream, int pipe = 0)
{
	if(!(c->instrumentation & 4) || !c->d_audit_seen || audit_words(c) * 32 < c->alloc_slots) return;
	const size_t n = (size_t)kNumSegments * q.seg_cap, n_seen = audit_words(c); // path ids are numbered over the whole batch, not over the chain's window
	hipLaunchKernelGGL(k_audit_poison, dim3((unsigned)((std::max(n, n_seen) + 255) / 256)), dim3(256), 0, stream, q.out_d, n, c->d_audit_seen + (size_t)pipe * audit_words(c), n_seen);
}
__global__ void k_audit_plant(float4 *out_d, const uint32_t *count) { if(count[0] >= 2u) out_d[1].w = out_d[0].w; } // (self-test of the detector: two slots, one path)
void audit_after(adypt_ctx *c, const QueueArgs &q, hipStream_t stream, int pipe = 0)
{
	if(!(c->instrumentation & 4) || !c->d_audit_seen || audit_words(c) * 32 < c->alloc_slots) return;
	if(c->audit_selftest) hipLaunchKernelGGL(k_audit_plant, dim3(1), dim3(1), 0, stream, q.out_d, (const uint32_t *)q.count_out);
	hipLaunchKernelGGL(k_audit_check, dim3((q.seg_cap + 255) / 256, kNumSegments), dim3(256), 0, stream, (const float4 *)q.out_d, (const uint32_t *)q.count_out, q.seg_cap, c->d_audit_seen + (size_t)pipe * audit_words(c),
					   (uint32_t)std::min<size_t>(audit_words(c) * 32, 0xffffffffu), &c->d_stats->audit_errors);
}

int ensure_ray_stats(adypt_ctx *c)
{
	if(!c->q.ray_stats) HIP_TRY(c, c->q.ray_stats.alloc((size_t)c->capacity * sizeof(RayStats)));
	return ADYPT_OK;
}

// update_config_args (OglPathTracer.cpp:214-225): pending parameters become active
int apply_params(adypt_ctx *c)
{
	c->params = c->pending;
	TRY_CREATE(configure_trace(c, c->params.stack_size));
	// cache slices for the tmpLifetime groups a batch of frames_in_flight frames can span (none for one frame at a time)
	const int life = std::max(1, c->params.tmp_lifetime);
	if(c->frames_in_flight > 1) TRY_CREATE(ensure_cache_slices(c, (c->frames_in_flight - 2) / life + 1));
	return load_shift(c);
}

}  // namespace

#include "scene_upload.hpp"
#include "frame_schedule.hpp"

namespace adypt {
// what every entry point of the noise statistics asks first: they are on, and the image has `min_spp` frames
int noise_ready(adypt_ctx *c, const char *who, int min_spp)
{
	if(!c->noise_stats) return fail(c, ADYPT_E_STATE, std::string(who) + ": the noise statistics are off (adypt_set_noise_stats)");
	if(c->spp < min_spp) return fail(c, ADYPT_E_STATE, std::string(who) + ": needs at least " + std::to_string(min_spp) + " spp");
	return ADYPT_OK;
}
}  // namespace adypt

namespace {

// ---- adaptive sampling: the block set of a pass (active_blocks.hpp) ----

// Every block active again (adypt_reset, adypt_trace_primary): passes are the owned blocks' and the device lists go back.  The cache image is
// written again before it is read: both callers restart the accumulation, whose first frame re-traces its camera rays.
void thaw_blocks(adypt_ctx *c)
{
	c->cache_stale = false;
	if(!c->ab.any_frozen()) return;
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream); // (passes enqueued earlier read the lists about to be freed)
	c->ab.thaw();
	c->pass_px = c->n_local_px; c->pass_image_px = c->n_image_px;
	c->adaptive = AdaptiveBuffers{};
}

// The owned blocks among blocks[0 .. n) (image block indices) stop at `spp` frames.  The lists go to the device, the compact shift image is
// gathered for the new active list, and the cache image is marked stale: its entries are in the order of the list that was.
int freeze_blocks(adypt_ctx *c, const int32_t *blocks, size_t n, int spp)
{
	std::vector<int32_t> mine; // (several devices: the list is the image's)
	for(size_t i = 0; i < n; ++i) if(spp >= 2 && c->ab.is_active(blocks[i])) mine.push_back(blocks[i]);
	if(mine.empty()) return ADYPT_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	drop_lookahead(c); // (refused before anything was traced; frames started ahead belong to the list that was)
	if(!c->adaptive)
	{
		// before the state changes: a failure here leaves the context as it was
		const hipError_t e = c->adaptive.alloc((size_t)c->n_local_blocks, (size_t)c->n_local_px);
		if(e != hipSuccess)
		{
			(void)hipGetLastError();
			return fail(c, e == hipErrorOutOfMemory ? ADYPT_E_OOM : ADYPT_E_HIP, std::string("adypt_trace_adaptive: ") + hipGetErrorString(e));
		}
	}
	// The device lists first, the host state afterwards: a failure on the way leaves a context whose passes are still the set's that was.  (If that set
	// had frozen blocks its lists are half overwritten by then: such a context refuses to trace, as one that lost its queues does.)
	ActiveBlocks next = c->ab;
	next.freeze(mine, spp);
	const size_t n_active = next.active.size();
	const int next_px = (int)(n_active * kBlockPixels);
	const int r = [&]() -> int {
		HIP_TRY(c, hipMemcpy(c->adaptive.frozen_at, next.frozen_at.data(), next.frozen_at.size() * sizeof(int32_t), hipMemcpyHostToDevice));
		if(n_active == 0) return ADYPT_OK;
		HIP_TRY(c, hipMemcpy(c->adaptive.blocks, next.active.data(), n_active * sizeof(int32_t), hipMemcpyHostToDevice));
		HIP_TRY(c, hipMemcpy(c->adaptive.slot, next.slot.data(), n_active * sizeof(int32_t), hipMemcpyHostToDevice));
		hipLaunchKernelGGL(k_gather_blocks<uint16_t>, dim3((unsigned)((next_px + 255) / 256)), dim3(256), 0, c->stream, (const uint16_t *)c->d_shift.get(), (const int32_t *)c->adaptive.slot,
		                   (uint16_t *)c->adaptive.shift.get(), next_px);
		HIP_TRY(c, hipGetLastError());
		return ADYPT_OK;
	}();
	if(r != ADYPT_OK)
	{
		if(c->ab.any_frozen()) { c->queues_ok = false; c->error += " (the block lists of the frozen set are lost: destroy the context)"; }
		else c->adaptive = AdaptiveBuffers{};
		return r;
	}
	c->ab = std::move(next);
	c->pass_px = next_px;
	c->pass_image_px = c->ab.active_image_px(c->width, c->height);
	c->cache_stale = true;
	return ADYPT_OK;
}

}  // namespace

namespace adypt {

namespace { std::atomic<bool> g_test_hooks{false}; }
bool test_hooks_enabled() { return g_test_hooks.load(std::memory_order_acquire); }

// The one place of csrc/device that reads the environment (tunables.hpp has the table).
Tunables read_tunables()
{
	Tunables t;
	auto num = [](const char *name, long lo, long hi, long unset) -> long {
		const char *v = getenv(name);
		if(!v || !*v) return unset;
		char *end = nullptr;
		const long x = strtol(v, &end, 10);
		if(end == v) return unset;
		return std::max(lo, std::min(hi, x));
	};
	auto flag = [&](const char *name, int unset) -> int { return num(name, 0, 1 << 30, unset) != 0 ? 1 : 0; };
	t.frames_in_flight = (int)num("ADYPT_FRAMES_IN_FLIGHT", 1, kMaxFramesInFlight, 0);
	t.pipeline = (int)num("ADYPT_PIPELINE", 1, kMaxPipes, kDefaultPipes);
	t.fused_bounces = flag("ADYPT_FUSED_BOUNCES", 1); t.first_fused = flag("ADYPT_FIRST_FUSED", 1); t.single_fused = flag("ADYPT_SINGLE_FUSED", 1);
	t.gen_deal = flag("ADYPT_GEN_DEAL", 1); t.shade_bin = flag("ADYPT_SHADE_BIN", 0); t.appearance_expand = flag("ADYPT_APPEARANCE_EXPAND", 0); t.single_overlap = flag("ADYPT_SINGLE_OVERLAP", 1);
	t.refill_min = (int)num("ADYPT_REFILL_MIN", 1, 64, 0); t.refill_min_primary = (int)num("ADYPT_REFILL_MIN_PRIMARY", 1, 64, 0);
	t.bite = (int)num("ADYPT_BITE", 1, 4096, 0); t.bite_primary = (int)num("ADYPT_BITE_PRIMARY", 1, 4096, 0);
	t.chunk = (int)num("ADYPT_CHUNK", 16, 4096, 0); t.endgame = (int)num("ADYPT_ENDGAME", 0, 1024, -1);
	t.shade_min = (int)num("ADYPT_SHADE_MIN", 1, 64, 0);
	t.rare_min = (int)num("ADYPT_RARE_MIN", 0, 64, -1); t.defer_max = (int)num("ADYPT_DEFER_MAX", 0, 64, -1);
	t.lds_stack_depth = (int)num("ADYPT_LDS_STACK_DEPTH", 1, kLdsStackMax, 0); t.trace_blocks_per_cu = (int)num("ADYPT_TRACE_BLOCKS_PER_CU", 1, 16, 0);
	t.path_blocks_per_cu = (int)num("ADYPT_PATH_BLOCKS_PER_CU", 1, 8, 0); t.path_lds_depth = (int)num("ADYPT_PATH_LDS_DEPTH", 1, kLdsStackMax, 0);
	t.path_verbose = flag("ADYPT_PATH_VERBOSE", 0);
	t.ref_triangles_max_mb = num("ADYPT_REF_TRIANGLES_MAX_MB", 0, 1 << 20, -1);
	if(const char *v = getenv("ADYPT_RCCL_LIB")) t.rccl_lib = v;
	if(const char *v = getenv("ADYPT_GATHER_TIMEOUT"))
	{
		// (a value that is not a number leaves the default in place: atof would read "abc" as 0 = no watchdog)
		char *end = nullptr;
		const double x = strtod(v, &end);
		if(end != v && *end == '\0' && x >= 0.0 && x <= 86400.0) t.gather_timeout_s = x;
		else fprintf(stderr, "[adypt] ADYPT_GATHER_TIMEOUT=\"%s\" is not a number of seconds in [0, 86400]: keeping %g s\n", v, t.gather_timeout_s);
	}
	if(test_hooks_enabled())
	{
		t.multi_shared_device = flag("ADYPT_MULTI_SHARED_DEVICE", 0) != 0;
		t.audit_selftest = flag("ADYPT_AUDIT_SELFTEST", 0) != 0;
		t.gather_stall_test = flag("ADYPT_GATHER_STALL_TEST", 0) != 0;
		t.root_card = flag("ADYPT_ROOT_CARD", 1);
		if(const char *v = getenv("ADYPT_COMM_TRANSPORT")) t.comm_transport_host = !strcmp(v, "host");
		if(const char *v = getenv("ADYPT_HOST_TRANSPORT_TIMEOUT")) t.host_transport_timeout_s = std::max(0.1, atof(v));
	}
	return t;
}

CtxInfo ctx_info(adypt_ctx *c)
{
	CtxInfo i;
	i.device = c->device; i.stream = c->stream; i.rank = c->rank; i.nranks = c->nranks; i.width = c->width; i.height = c->height;
	i.n_local_px = c->n_local_px; i.accum = c->d_accum;
	return i;
}
void ctx_set_error(adypt_ctx *c, const std::string &msg) { c->error = msg; }
Attachment &ctx_attachment(adypt_ctx *c, AttachKind kind) { return c->attached[kind]; }
int ctx_adaptive_ready(adypt_ctx *c, const char *fn)
{
	TRY_CREATE(noise_ready(c, fn, 0));
	if(c->lookahead || c->ahead_count > 0)
		return fail(c, ADYPT_E_STATE, std::string(fn) + ": look-ahead is enabled or frames are parked ahead: they belong to a block set that a check may change (adypt_set_lookahead(ctx, 0))");
	return ADYPT_OK;
}
int ctx_freeze_blocks(adypt_ctx *c, const int32_t *blocks, size_t n, int spp) { return freeze_blocks(c, blocks, n, spp); }
int ctx_plan_ready(adypt_ctx *c, const char *fn)
{
	TRY_CREATE(ctx_adaptive_ready(c, fn));
	if(!c->have_camera) return fail(c, ADYPT_E_STATE, std::string(fn) + ": call adypt_set_camera first");
	if(!c->queues_ok) return fail(c, ADYPT_E_STATE, std::string(fn) + ": the context lost its ray queues (failed adypt_set_frames_in_flight)");
	if(c->ab.any_frozen()) return fail(c, ADYPT_E_STATE, std::string(fn) + ": blocks are frozen (adypt_reset first)");
	if(c->spp != 0) return fail(c, ADYPT_E_STATE, std::string(fn) + ": the plan is made before the first sample of a pose (adypt_reset first: adypt_get_spp is " + std::to_string(c->spp) + ")");
	return ADYPT_OK;
}
int ctx_spp(adypt_ctx *c) { return c->spp; }

// ---- what the denoiser (denoise.hip) needs of a context ----
int ctx_denoise_ready(adypt_ctx *c, const char *fn, int min_spp)
{
	const std::string too_few = min_spp >= 2 ? ": needs at least 2 spp in every block (the variance of a pixel's mean is not defined below)" : ": needs at least 1 spp in every block";
	TRY_CREATE(noise_ready(c, fn, 0));
	if(c->view_type != 3) return fail(c, ADYPT_E_STATE, std::string(fn) + ": the image is not path-traced (the last frame was a primary-ray viewer's)");
	for(size_t i = 0; i < c->ab.owned.size(); ++i)
		if(c->ab.spp_of(i, c->spp) < min_spp) return fail(c, ADYPT_E_STATE, std::string(fn) + too_few);
	if(c->ab.owned.empty() && c->spp < min_spp) return fail(c, ADYPT_E_STATE, std::string(fn) + too_few);
	return ADYPT_OK;
}
DenoiseInputs ctx_denoise_inputs(adypt_ctx *c)
{
	DenoiseInputs in;
	in.accum = c->d_accum; in.moments = (const float2 *)c->d_noise_moments.get(); in.blocks = c->d_local_blocks;
	in.n_blocks = c->n_local_blocks; in.block_index = c->local_blocks;
	in.block_spp.resize(c->ab.owned.size());
	for(size_t i = 0; i < in.block_spp.size(); ++i) in.block_spp[i] = c->ab.spp_of(i, c->spp);
	return in;
}
// Albedo, normal, position (the viewer colours of types 0, 4, 5) and the primary hit of the pixel-centre camera ray of every owned pixel, under the
// current camera and parameters, into the caller's four block-major images (each max(owned pixels, 64) float4): three launches of the viewer
// instance of k_trace_camera over the OWNED blocks, on the context's stream behind the frames.  Nothing of the context's own changes: not the image,
// not the primary-hit cache, not view_type / spp / the frozen set / the frames parked ahead.
int ctx_capture_guides(adypt_ctx *c, const char *fn, float4 *albedo, float4 *normal, float4 *position, float4 *hits)
{
	if(!c->have_camera) return fail(c, ADYPT_E_STATE, std::string(fn) + ": call adypt_set_camera first");
	if(!c->queues_ok) return fail(c, ADYPT_E_STATE, std::string(fn) + ": the context lost its ray queues (failed adypt_set_frames_in_flight)");
	if(c->n_local_px == 0) return ADYPT_OK;
	HIP_TRY(c, hipSetDevice(c->device));
	FrameArgs f;
	fill_frame(c, &f);
	f.n_local_px = c->n_local_px; f.spp = 0;
	float4 *const image[3] = {albedo, normal, position};
	const int type[3] = {0, 4, 5};
	for(int k = 0; k < 3; ++k)
	{
		PixelArgs px;
		fill_pixels(c, &px);
		px.accum = image[k]; px.cache = hits; px.cache_next = hits; px.shift = c->d_shift;
		TRY_CREATE(launch_trace_camera(c, c->pipes[0], full_window(c), f, px, 0, false, type[k], true));
	}
	return ADYPT_OK;
}
CtxCamera ctx_camera(adypt_ctx *c)
{
	CtxCamera cam;
	memcpy(cam.origin, c->origin, 12); memcpy(cam.inv_proj, c->inv_proj, 64); memcpy(cam.inv_view, c->inv_view, 64);
	return cam;
}
// The context's ray queues for rounds of rays another unit writes itself (the denoiser's chain through mirrors and glass).  Towards frames started
// ahead it behaves as adypt_trace_rays does: they work in a window of these queues and are waited for; frames parked ahead live elsewhere and stay.
// The counters of every round are cleared on the context's stream before it returns.
int ctx_ray_queues(adypt_ctx *c, const char *fn, CtxRayQueues *q)
{
	if(!c->queues_ok) return fail(c, ADYPT_E_STATE, std::string(fn) + ": the context lost its ray queues (failed adypt_set_frames_in_flight)");
	HIP_TRY(c, hipSetDevice(c->device));
	drop_rolling(c);
	static_assert(sizeof(c->d_counters->count[0]) == sizeof(uint32_t) * kNumSegments * kCursorStride, "one round of counters");
	for(int i = 0; i < 2; ++i) { q->o[i] = c->q.o[i]; q->d[i] = c->q.d[i]; }
	q->hit = c->q.hit;
	q->count = c->d_counters->count[0];
	q->rounds = kMaxBounce + 1; q->round_stride = kNumSegments * kCursorStride; q->seg_stride = kCursorStride;
	q->segments = kNumSegments; q->seg_cap = c->seg_cap;
	q->tmin = c->params.ray_tmin;
	clear_counters(c, c->d_counters, 1, c->stream);
	HIP_TRY(c, hipGetLastError());
	return ADYPT_OK;
}
// the closest hits of the rays of round `round` in queue `parity` (the count of every segment where ctx_ray_queues says) into the hit queue: one launch
// of k_trace on the context's stream, no host sync
int ctx_trace_queue(adypt_ctx *c, int parity, int round)
{
	return launch_trace(c, c->pipes[0], full_window(c), parity, c->d_counters->count[round], c->d_counters->cursor[round], c->params.stack_size, false, nullptr);
}

// ---- what the refit (refit.hip) needs of a context ----
CtxScene ctx_scene(adypt_ctx *c)
{
	return CtxScene{c->d_nodes, c->d_woop, c->d_triangles, c->d_tri_indices, c->n_nodes, c->n_refs, c->n_tris, kTriFloat4};
}
int ctx_expand_references(adypt_ctx *c)
{
	const size_t n16 = (size_t)c->n_refs * kTriFloat4;
	if(!c->d_ref_triangles || !n16) return ADYPT_OK;
	hipLaunchKernelGGL(k_expand_references, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, c->stream, (const float4 *)c->d_triangles, (const int32_t *)c->d_tri_indices, (size_t)c->n_refs, (float4 *)c->d_ref_triangles);
	HIP_TRY(c, hipGetLastError());
	return ADYPT_OK;
}
int ctx_refresh_root_card(adypt_ctx *c)
{
	if(!c->d_root_card) HIP_TRY(c, c->d_root_card.alloc(sizeof(RootCard)));
	hipLaunchKernelGGL(k_root_card, dim3(1), dim3(64), 0, c->stream, (const uint4 *)c->d_nodes, c->tun.root_card, (RootCard *)c->d_root_card);
	HIP_TRY(c, hipGetLastError());
	return ADYPT_OK;
}
int ctx_drain(adypt_ctx *c)
{
	HIP_TRY(c, hipSetDevice(c->device));
	for(int k = 0; k < kMaxPipes; ++k) if(c->pipes[k].stream) HIP_TRY(c, hipStreamSynchronize(c->pipes[k].stream));
	harvest_events(c);
	return ADYPT_OK; // (a stack overflow of those frames stays for adypt_wait to report)
}
// ---- what the rebuild (build.hip) needs of a context ----
// The tree is replaced by one built in the caller's buffers (the context is drained, the buffers' contents are complete on the context's stream): the
// node, index and Woop arrays are taken, the old ones go back with the caller's owners; what adypt_create derived from the tree's size is derived again
// (the per-reference copy of the records, the launch geometry of the traversal); the context is left as adypt_reset leaves it.  What can be refused
// comes first: after a failure the old tree is in place and usable.
int ctx_replace_bvh(adypt_ctx *c, Buffer<uint4> *nodes, Buffer<int32_t> *tri_indices, Buffer<float4> *woop, int64_t n_nodes, int64_t n_refs)
{
	return ctx_replace_geometry(c, nullptr, nodes, tri_indices, woop, n_nodes, n_refs);
}
// ---- what replacing the triangles (geometry.hip) needs of a context ----
CtxMaterials ctx_materials(adypt_ctx *c)
{
	return CtxMaterials{(const float4 *)c->d_materials, c->n_mats, c->n_tex, kMatFloat4, c->tun.shade_bin != 0, (const uint32_t *)c->d_texels};
}
// ---- what changing the appearance (appearance.hip) needs of a context ----
CtxAppearance ctx_appearance(adypt_ctx *c)
{
	return CtxAppearance{c->d_materials, c->d_texels, c->tun.shade_bin ? c->d_tri_class.get() : nullptr, c->d_ref_triangles, c->tex_desc.data(), c->n_mats, c->n_texels, c->n_tex, kMatFloat4,
	                     c->d_materials.bytes() + c->d_texels.bytes(), c->tun.appearance_expand != 0};
}
void ctx_replace_appearance(adypt_ctx *c, Buffer<float4> *materials, int64_t n_mats, Buffer<uint32_t> *texels, std::vector<int32_t> *tex_desc, int64_t n_texels)
{
	std::swap(c->d_materials, *materials);
	c->n_mats = n_mats;
	if(!texels) return;
	std::swap(c->d_texels, *texels);
	c->tex_desc.swap(*tex_desc);
	c->n_tex = (int)(c->tex_desc.size() / 4);
	c->n_texels = n_texels;
}
void ctx_set_create_error(const std::string &msg) { g_create_error = msg; }
// ctx_replace_bvh, and with `geometry` the triangles the tree was built of as well (packed by k_pack_triangles, complete on the context's stream): the
// records, the class bytes where the context keeps them, and the count are taken in the same step as the tree, and go back with it when the new tree is refused.
int ctx_replace_geometry(adypt_ctx *c, NewGeometry *geometry, Buffer<uint4> *nodes, Buffer<int32_t> *tri_indices, Buffer<float4> *woop, int64_t n_nodes, int64_t n_refs)
{
	HIP_TRY(c, hipSetDevice(c->device));
	Buffer<float4> ref;
	size_t ref_bytes;
	if(wants_reference_triangles(c, n_refs, &ref_bytes) && ref.alloc(ref_bytes) != hipSuccess) (void)hipGetLastError(); // (left empty: k_path remaps, as after adypt_create)
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	int64_t other_nodes = n_nodes, other_refs = n_refs, other_tris = geometry ? geometry->n_tris : c->n_tris;
	auto swap_all = [&] {
		std::swap(c->d_nodes, *nodes); std::swap(c->d_tri_indices, *tri_indices); std::swap(c->d_woop, *woop); std::swap(c->d_ref_triangles, ref);
		if(geometry)
		{
			std::swap(c->d_triangles, *geometry->records);
			if(c->tun.shade_bin) std::swap(c->d_tri_class, *geometry->classes);
		}
		std::swap(c->n_nodes, other_nodes); std::swap(c->n_refs, other_refs); std::swap(c->n_tris, other_tris);
	};
	swap_all();
	const int r = configure_trace(c, c->params.stack_size);
	if(r != ADYPT_OK)
	{
		const std::string why = c->error;
		swap_all();
		(void)configure_trace(c, c->params.stack_size);
		c->error = why;
		return r;
	}
	const int e = ctx_expand_references(c);
	if(e != ADYPT_OK) return e;
	TRY_CREATE(ctx_refresh_root_card(c)); // (the new tree's node 0: behind k_emit and the refit of every rebuild method, which ran on this stream)
	HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the old per-reference copy goes with `ref`)
	return adypt_reset(c);
}
}  // namespace adypt

namespace {

// First line of a C-ABI function that touches the device: the context's device current (a process may hold contexts on several devices) and,
// DRAINED, everything enqueued on the context's stream finished.  Which of the two an entry point takes is its own (include/adypt_hip.h).
#define ENTER(c) HIP_TRY(c, hipSetDevice(c->device))
#define ENTER_DRAINED(c) do { ENTER(c); HIP_TRY(c, hipStreamSynchronize(c->stream)); } while(0)

int read_device_stats(adypt_ctx *c, DeviceStats *st)
{
	ENTER_DRAINED(c);
	HIP_TRY(c, hipMemcpy(st, c->d_stats, sizeof(*st), hipMemcpyDeviceToHost));
	return ADYPT_OK;
}

// ---- the steps of adypt_create ----

int create_streams(adypt_ctx *c)
{
	for(int k = 0; k < kMaxPipes; ++k) HIP_TRY(c, hipStreamCreateWithFlags(c->pipes[k].stream.out(), hipStreamNonBlocking));
	c->stream = c->pipes[0].stream;
	for(int k = 0; k < kMaxPipes; ++k) HIP_TRY(c, hipEventCreateWithFlags(c->pipes[k].done.out(), hipEventDisableTiming));
	HIP_TRY(c, hipEventCreateWithFlags(c->fork_ev.out(), hipEventDisableTiming));
	for(int s = 0; s < 2; ++s) HIP_TRY(c, hipEventCreateWithFlags(c->roll_ready[s].out(), hipEventDisableTiming));
	return ADYPT_OK;
}

void apply_tunables(adypt_ctx *c)
{
	c->tun = read_tunables();
	c->pipeline = c->tun.pipeline;
	const Tunables &t = c->tun;
	if(t.refill_min > 0) c->refill_min = c->refill_min_primary = (uint32_t)t.refill_min;
	if(t.refill_min_primary > 0) c->refill_min_primary = (uint32_t)t.refill_min_primary;
	c->deal_chunks = t.gen_deal; c->first_fused = t.first_fused; c->fused_bounces = t.fused_bounces; c->single_fused = t.single_fused;
	c->audit_selftest = t.audit_selftest; c->single_overlap = t.single_overlap;
	if(t.shade_min > 0) c->shade_min = (uint32_t)t.shade_min;
	if(t.rare_min >= 0) c->rare_min = (uint32_t)t.rare_min;
	if(t.defer_max >= 0) c->defer_max = (uint32_t)t.defer_max;
	if(t.chunk > 0) c->chunk = (uint32_t)t.chunk;
	if(t.endgame >= 0) c->endgame = (uint32_t)t.endgame;
	if(t.bite > 0) c->bite = c->bite_primary = (uint32_t)t.bite;
	if(t.bite_primary > 0) c->bite_primary = (uint32_t)t.bite_primary;
}

// the sizes of the scene and the pixel-tile shard: which 32x32 blocks of the image are this context's
void set_shard(adypt_ctx *c, const adypt_scene_desc *d)
{
	c->n_nodes = d->n_nodes; c->n_refs = d->n_refs; c->n_tris = d->n_tris; c->n_mats = d->n_mats; c->n_tex = d->n_textures;
	c->width = d->width; c->height = d->height; c->rank = d->tile_rank; c->nranks = d->tile_nranks;
	c->blocks_x = (c->width + kBlockDim - 1) / kBlockDim; c->blocks_y = (c->height + kBlockDim - 1) / kBlockDim;
	c->local_blocks = owned_blocks(c->width, c->height, c->rank, c->nranks);
	c->n_local_blocks = (int)c->local_blocks.size();
	c->n_local_px = c->n_local_blocks * kBlockPixels;
	c->n_image_px = 0;
	for(int32_t blk : c->local_blocks)
	{
		const int bx = blk % c->blocks_x, by = blk / c->blocks_x;
		c->n_image_px += (int64_t)std::min(kBlockDim, c->width - bx * kBlockDim) * (int64_t)std::min(kBlockDim, c->height - by * kBlockDim);
	}
	c->ab.reset(c->local_blocks); // every block active: a pass is the owned blocks'
	c->pass_px = c->n_local_px; c->pass_image_px = c->n_image_px;
}

// per-pixel images, ray queues, Sobol staging, counters and statistics
int alloc_frame_state(adypt_ctx *c)
{
	const size_t npx = (size_t)std::max(c->n_local_px, 64);
	HIP_TRY(c, c->d_accum.alloc(npx * sizeof(float4)));
	HIP_TRY(c, c->d_cache.alloc(npx * sizeof(float4)));
	HIP_TRY(c, c->d_shift.alloc(npx * 2));
	HIP_TRY(c, hipMemset(c->d_accum, 0, npx * sizeof(float4)));
	HIP_TRY(c, hipMemset(c->d_cache, 0xff, npx * sizeof(float4)));
	HIP_TRY(c, hipMemset(c->d_shift, 0, npx * 2));
	{
		// frames in flight: enough consecutive frames per wavefront pass to keep ~64 Mi paths in flight (32 frames of a
		// 1080p image, 128 frames = the maximum for the 260 k-pixel tile shard of an 8-GPU run): the drain of a persistent
		// launch (its longest rays) is amortised over more work; ADYPT_FRAMES_IN_FLIGHT overrides
		int fif = (int)std::min<size_t>(kMaxFramesInFlight, std::max<size_t>(1, ((size_t)64 << 20) / npx));
		if(c->tun.frames_in_flight > 0) fif = std::min(kMaxFramesInFlight, c->tun.frames_in_flight);
		TRY_CREATE(alloc_queues(c, fif));
	}
	HIP_TRY(c, c->d_sobol.alloc((size_t)kMaxFramesInFlight * 64 * sizeof(float)));
	for(int i = 0; i < adypt_ctx::kSobolSlots; ++i) // allocated here, not lazily: nothing is allocated while frames are traced
	{
		HIP_TRY(c, c->h_sobol[i].alloc((size_t)kMaxFramesInFlight * 64 * sizeof(float), hipHostMallocDefault));
		HIP_TRY(c, hipEventCreateWithFlags(c->sobol_done[i].out(), hipEventDisableTiming));
	}
	HIP_TRY(c, c->d_counters.alloc(sizeof(FrameCounters) * kMaxPipes));
	for(int k = 0; k < kMaxPipes; ++k) c->pipes[k].counters = c->d_counters + k;
	HIP_TRY(c, c->d_stats.alloc(sizeof(DeviceStats)));
	HIP_TRY(c, hipMemset(c->d_counters, 0, sizeof(FrameCounters) * kMaxPipes));
	HIP_TRY(c, c->d_camera_cursors.alloc(sizeof(uint32_t) * (2 * kNumSegments + 1) * kCursorStride));
	HIP_TRY(c, hipMemset(c->d_camera_cursors, 0, sizeof(uint32_t) * (2 * kNumSegments + 1) * kCursorStride));
	HIP_TRY(c, hipMemset(c->d_stats, 0, sizeof(DeviceStats)));
	HIP_TRY(c, c->h_overflow.alloc(sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent));
	*c->h_overflow = 0u;
	uint32_t *const h_overflow = c->h_overflow;
	HIP_TRY(c, hipMemcpy(&c->d_stats->host_overflow, &h_overflow, sizeof(uint32_t *), hipMemcpyHostToDevice));
	return ADYPT_OK;
}

int create_steps(adypt_ctx *c, const adypt_scene_desc *d)
{
	ENTER(c);
	TRY_CREATE(create_streams(c));
	apply_tunables(c);
	hipDeviceProp_t prop;
	HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
	c->num_cus = prop.multiProcessorCount;
	if(prop.maxSharedMemoryPerMultiProcessor >= 64 * 1024) c->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
	set_shard(c, d);
	TRY_CREATE(upload_scene(c, d));
	TRY_CREATE(alloc_frame_state(c));
	// defaults of InstanceConfig::PT (src/InstanceConfig.hpp:21-27), seed 0
	c->pending.stack_size = 12; c->pending.max_bounce = 5; c->pending.subpixel = 8; c->pending.tmp_lifetime = 16;
	c->pending.ray_tmin = 0.0001f; c->pending.clamp = 4.0f; c->pending.sun[0] = c->pending.sun[1] = c->pending.sun[2] = 0.0f;
	c->pending.shift_seed = 0;
	TRY_CREATE(apply_params(c));
	HIP_TRY(c, hipDeviceSynchronize()); // the uploads / memsets above ran on the legacy stream
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return ADYPT_OK;
}

}  // namespace

extern "C" {

int adypt_abi_version(void) { return ADYPT_ABI_VERSION; }

int adypt_enable_test_hooks(uint64_t magic)
{
	if(magic != ADYPT_TEST_HOOKS_MAGIC) return ADYPT_E_INVALID;
	g_test_hooks.store(true, std::memory_order_release);
	return ADYPT_OK;
}
int adypt_test_hooks_enabled(void) { return test_hooks_enabled() ? 1 : 0; }

const char *adypt_last_error(const adypt_ctx *ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int64_t adypt_shard_block_count(int width, int height, int rank, int nranks)
{
	if(width <= 0 || height <= 0 || nranks <= 0 || rank < 0 || rank >= nranks) return -1;
	return (int64_t)owned_blocks(width, height, rank, nranks).size();
}

int adypt_untile_host(int width, int height, int rank, int nranks, const float *local_rgba, float *rgb)
{
	if(width <= 0 || height <= 0 || nranks <= 0 || rank < 0 || rank >= nranks || !local_rgba || !rgb) return ADYPT_E_INVALID;
	for_each_local_pixel(owned_blocks(width, height, rank, nranks), width, height, [&](size_t L, int x, int y) {
		const float *s = local_rgba + L * 4;
		float *o = rgb + ((size_t)y * width + x) * 3;
		o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
	});
	return ADYPT_OK;
}

int adypt_create(adypt_ctx **out, const adypt_scene_desc *d)
{
	g_create_error.clear();
	if(!out || !d) { g_create_error = "adypt_create: null argument"; return ADYPT_E_INVALID; }
	*out = nullptr;
	if(!d->nodes || !d->tri_indices || !d->triangles || d->n_nodes <= 0 || d->n_refs < 0 || d->n_tris <= 0 || d->n_mats < 0 ||
	   d->width <= 0 || d->height <= 0 || d->n_textures < 0 || (d->n_mats > 0 && !d->materials) || (d->n_textures > 0 && !d->textures) ||
	   d->tile_nranks <= 0 || d->tile_rank < 0 || d->tile_rank >= d->tile_nranks)
	{ g_create_error = "adypt_create: inconsistent scene description"; return ADYPT_E_INVALID; }
	if((int64_t)d->width * d->height > (int64_t)1 << 30) { g_create_error = "adypt_create: image too large"; return ADYPT_E_INVALID; }
	{
		std::string why;
		if(!validate_bvh(*d, &why)) { g_create_error = "adypt_create: invalid BVH arrays: " + why; return ADYPT_E_INVALID; }
	}
	int n_dev = 0;
	if(hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { g_create_error = "adypt_create: no HIP device available (this library has no CPU path)"; return ADYPT_E_NO_DEVICE; }
	if(d->device < 0 || d->device >= n_dev) { g_create_error = "adypt_create: device ordinal out of range"; return ADYPT_E_INVALID; }

	adypt_ctx *c = new adypt_ctx();
	c->device = d->device;
	const int r = create_steps(c, d);
	if(r != ADYPT_OK) { g_create_error = c->error; adypt_destroy(c); return r; }
	*out = c;
	return ADYPT_OK;
}

void adypt_destroy(adypt_ctx *c)
{
	if(!c) return;
	(void)hipSetDevice(c->device);
	for(int k = 0; k < kMaxPipes; ++k) if(c->pipes[k].stream) (void)hipStreamSynchronize(c->pipes[k].stream);
	for(Attachment &a : c->attached) a.reset(); // the communicator, the denoiser, the refit
	delete c; // every member releases itself, the streams and events last (context.hpp)
}

int adypt_set_params(adypt_ctx *c, const adypt_pt_params *p)
{
	if(!c || !p) return ADYPT_E_INVALID;
	// subpixel * subpixel is an int in the kernels (pathtracer.glsl:207 does the same in GLSL int): 46340^2 < 2^31
	if(p->stack_size < 1 || p->stack_size > 64 || p->max_bounce < 1 || p->max_bounce > kMaxBounce || p->subpixel < 1 || p->subpixel > 46340 || p->tmp_lifetime < 1)
		return fail(c, ADYPT_E_INVALID, "adypt_set_params: stackSize must be in [1,64], maxBounce in [1,32], subpixel in [1,46340], tmpLifetime >= 1");
	c->pending = *p;
	c->have_params = true;
	if(!c->pt_started)
	{
		ENTER(c); // (not drained: each step of apply_params that replaces something in use waits for its users itself)
		return apply_params(c);
	}
	return ADYPT_OK;
}

int adypt_set_camera(adypt_ctx *c, const float origin[3], const float inv_proj[16], const float inv_view[16])
{
	if(!c || !origin || !inv_proj || !inv_view) return ADYPT_E_INVALID;
	memcpy(c->origin, origin, 12); memcpy(c->inv_proj, inv_proj, 64); memcpy(c->inv_view, inv_view, 64);
	c->have_camera = true;
	drop_lookahead(c); // frames traced ahead saw the previous camera
	return ADYPT_OK;
}

int adypt_reset(adypt_ctx *c)
{
	if(!c) return ADYPT_E_INVALID;
	c->pt_started = false;
	c->spp = 0;
	drop_lookahead(c);
	thaw_blocks(c);
	return ADYPT_OK;
}

int adypt_set_lookahead(adypt_ctx *c, int enabled)
{
	if(!c) return ADYPT_E_INVALID;
	c->lookahead = enabled ? 1 : 0;
	if(!enabled) drop_lookahead(c);
	return ADYPT_OK;
}

int adypt_get_lookahead_frames(const adypt_ctx *c) { return c ? c->ahead_count : ADYPT_E_INVALID; }

int adypt_get_spp(const adypt_ctx *c) { return c ? c->spp : ADYPT_E_INVALID; }

int adypt_set_instrumentation(adypt_ctx *c, int flags)
{
	if(!c) return ADYPT_E_INVALID;
	c->instrumentation = flags;
	if(flags & 4) { ENTER(c); TRY_CREATE(ensure_audit(c)); }
	if(flags & 1)
	{
		// a pool of event pairs for the kernel timing, created here rather than while frames are being traced
		ENTER(c);
		while(c->free_events.size() + c->events.size() < 96)
		{
			EventPair p;
			HIP_TRY(c, hipEventCreate(p.a.out()));
			HIP_TRY(c, hipEventCreate(p.b.out()));
			c->free_events.push_back(std::move(p));
		}
	}
	return ADYPT_OK;
}

int adypt_set_sun_visibility(adypt_ctx *c, int enabled, const float dir[3])
{
	if(!c) return ADYPT_E_INVALID;
	float d[3] = {0.6f, 1.0f, 0.2f}; // the direction of the reference's commented-out query (pathtracer.glsl:132)
	if(dir) memcpy(d, dir, sizeof(d));
	const float len2 = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]));
	if(!(len2 > 0.0f) || !(len2 < INFINITY)) return fail(c, ADYPT_E_INVALID, "adypt_set_sun_visibility: direction must be finite and non-zero");
	const float inv = 1.0f / sqrtf(len2); // normalize() in the canonical arithmetic (canon_math.hpp normalize3)
	ENTER_DRAINED(c);
	c->sun_dir[0] = d[0] * inv; c->sun_dir[1] = d[1] * inv; c->sun_dir[2] = d[2] * inv;
	c->sun_visibility = enabled ? 1 : 0;
	drop_lookahead(c);
	return ADYPT_OK;
}

int adypt_set_frames_in_flight(adypt_ctx *c, int n)
{
	if(!c) return ADYPT_E_INVALID;
	if(n < 1 || n > kMaxFramesInFlight) return fail(c, ADYPT_E_INVALID, "adypt_set_frames_in_flight: n_frames must be in [1, " + std::to_string(kMaxFramesInFlight) + "]");
	ENTER_DRAINED(c);
	if(n == c->frames_in_flight && c->queues_ok) return ADYPT_OK;
	drop_lookahead(c); // the parked samples live in the buffers about to be reallocated
	int r = alloc_queues(c, n);
	if(r == ADYPT_OK && (c->instrumentation & 4)) r = ensure_audit(c);
	return r;
}

int adypt_get_frames_in_flight(const adypt_ctx *c) { return c ? c->frames_in_flight : ADYPT_E_INVALID; }

int adypt_set_pipeline(adypt_ctx *c, int n_pipes)
{
	if(!c) return ADYPT_E_INVALID;
	if(n_pipes < 1 || n_pipes > kMaxPipes) return fail(c, ADYPT_E_INVALID, "adypt_set_pipeline: n_pipes must be in [1, " + std::to_string(kMaxPipes) + "]");
	c->pipeline = n_pipes; // takes effect with the next batch; nothing in flight depends on it
	return ADYPT_OK;
}

int adypt_get_pipeline(const adypt_ctx *c) { return c ? c->pipeline : ADYPT_E_INVALID; }

int adypt_set_fused_bounces(adypt_ctx *c, int enabled)
{
	if(!c) return ADYPT_E_INVALID;
	c->fused_bounces = enabled ? 1 : 0; // takes effect with the next batch; both pipelines leave the same image and the same state behind
	return ADYPT_OK;
}

int adypt_get_fused_bounces(const adypt_ctx *c) { return c ? (c->last_batch_fused ? 1 : 0) : ADYPT_E_INVALID; }

int adypt_trace_primary(adypt_ctx *c, int viewer_type)
{
	if(!c) return ADYPT_E_INVALID;
	if(!c->have_camera) return fail(c, ADYPT_E_STATE, "adypt_trace_primary: call adypt_set_camera first");
	if(!c->queues_ok) return fail(c, ADYPT_E_STATE, "adypt_trace_primary: the context lost its ray queues (failed adypt_set_frames_in_flight)");
	ENTER(c);
	// Trace(false): leaves path-tracing mode (OglPathTracer.cpp:53-58)
	c->pt_started = false; c->spp = 0;
	drop_lookahead(c);
	thaw_blocks(c); // a viewer frame is of every pixel
	c->view_type = viewer_type;
	TRY_CREATE(apply_params(c));
	if(c->n_local_px == 0) return ADYPT_OK; // a tile shard that owns no 32x32 block (more ranks than block diagonals): nothing to render
	FrameArgs f; SceneArgs sc; PixelArgs px;
	fill_frame(c, &f); fill_scene(c, &sc); fill_pixels(c, &px);
	const Pipe &pipe = c->pipes[0];
	const QueueWindow win = full_window(c);
	// camera rays -> traversal -> cache image and the viewer's colour of every pixel (primaryray.glsl:46-94): one launch is the whole call
	TRY_CREATE(launch_trace_camera(c, pipe, win, f, px, 0, (c->instrumentation & 2) != 0, viewer_type));
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	harvest_events(c);
	return check_async_errors(c);
}

int adypt_wait(adypt_ctx *c)
{
	if(!c) return ADYPT_E_INVALID;
	ENTER_DRAINED(c);
	harvest_events(c);
	return check_async_errors(c);
}

int adypt_trace_spp(adypt_ctx *c, int n_spp)
{
	int r = adypt_trace_spp_async(c, n_spp);
	return r != ADYPT_OK ? r : adypt_wait(c);
}

int adypt_trace_spp_async(adypt_ctx *c, int n_spp)
{
	if(!c || n_spp < 0) return ADYPT_E_INVALID;
	if(!c->have_camera) return fail(c, ADYPT_E_STATE, "adypt_trace_spp: call adypt_set_camera first");
	if(!c->queues_ok) return fail(c, ADYPT_E_STATE, "adypt_trace_spp: the context lost its ray queues (failed adypt_set_frames_in_flight)");
	ENTER(c);
	if(c->pass_px == 0)
	{
		// a tile shard that owns no 32x32 block (more ranks than block diagonals, e.g. 64x36 on 4 ranks), or one whose blocks are all frozen
		// (adypt_trace_adaptive): the frame counter and the parameter hand-over advance like everywhere else, no kernel runs (they would
		// divide by n_local_px)
		if(n_spp > 0 && !c->pt_started)
		{
			TRY_CREATE(apply_params(c));
			c->spp = 0; c->pt_started = true; c->view_type = 3;
		}
		c->spp += n_spp;
		return ADYPT_OK;
	}
	for(int remaining = n_spp; remaining > 0;)
	{
		int r, done;
		if(c->ahead_count > 0) r = hand_out_parked(c, done = std::min(remaining, c->ahead_count));
		else
		{
			if(!c->pt_started && (r = start_path_tracing(c)) != ADYPT_OK) return r;
			const PassPlan p = plan_pass(plan_input(c, remaining));
			r = p.kind == PassPlan::Rolling ? trace_rolling_frame(c, p, remaining > 1) : enqueue_batch(c, p);
			done = p.hand_out;
			if(r == ADYPT_OK) c->cache_stale = false; // (the pass has written the cache image of every group it touches for the current block set)
		}
		if(r != ADYPT_OK) return r;
		remaining -= done;
	}
	return ADYPT_OK; // everything is enqueued on the context's stream; adypt_wait collects errors and kernel timings
}

int adypt_read_radiance(adypt_ctx *c, float *rgb)
{
	if(!c || !rgb) return ADYPT_E_INVALID;
	// the context's stream is non-blocking: a legacy-stream copy is not ordered after the frames enqueued by
	// adypt_trace_spp_async, so wait for them here (include/adypt_hip.h: entry points that read results synchronise)
	ENTER_DRAINED(c);
	if(c->n_local_px == 0) return ADYPT_OK; // a shard that owns no block: nothing of the image is this context's
	std::vector<float> local((size_t)c->n_local_px * 4);
	HIP_TRY(c, hipMemcpy(local.data(), c->d_accum, local.size() * sizeof(float), hipMemcpyDeviceToHost));
	return adypt_untile_host(c->width, c->height, c->rank, c->nranks, local.data(), rgb);
}

int adypt_read_display(adypt_ctx *c, uint8_t *rgba8)
{
	if(!c || !rgba8) return ADYPT_E_INVALID;
	ENTER(c); // (not drained, on purpose: the display transform and the copy are enqueued BEHIND the frames on the context's stream, then waited for)
	if(c->n_local_px == 0) return ADYPT_OK;
	if(!c->d_display) HIP_TRY(c, c->d_display.alloc((size_t)c->n_local_px * sizeof(uint32_t))); // once: the size never changes
	hipLaunchKernelGGL(k_display, dim3((c->n_local_px + 255) / 256), dim3(256), 0, c->stream, (const float4 *)c->d_accum, c->n_local_px, c->view_type, c->d_display);
	std::vector<uint32_t> local((size_t)c->n_local_px);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipMemcpyAsync(local.data(), c->d_display, local.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	for_each_local_pixel(c->local_blocks, c->width, c->height, [&](size_t L, int x, int y) { memcpy(rgba8 + ((size_t)y * c->width + x) * 4, &local[L], 4); });
	return ADYPT_OK;
}

int adypt_read_hits(adypt_ctx *c, int32_t *tri, float *uv)
{
	if(!c || !tri || !uv) return ADYPT_E_INVALID;
	ENTER_DRAINED(c); // see adypt_read_radiance
	if(c->n_local_px == 0) return ADYPT_OK;
	if(c->ab.any_frozen()) return fail(c, ADYPT_E_STATE, "adypt_read_hits: blocks are frozen (adypt_trace_adaptive): the cached primary hits are kept in the order of the active blocks");
	std::vector<float> local((size_t)c->n_local_px * 4);
	HIP_TRY(c, hipMemcpy(local.data(), c->d_cache, local.size() * sizeof(float), hipMemcpyDeviceToHost));
	for_each_local_pixel(c->local_blocks, c->width, c->height, [&](size_t L, int x, int y) {
		const size_t p = (size_t)y * c->width + x;
		memcpy(&tri[p], &local[L * 4], 4);
		uv[p * 2] = local[L * 4 + 1]; uv[p * 2 + 1] = local[L * 4 + 2];
	});
	return ADYPT_OK;
}

// ---- noise statistics (noise.hpp) ----

int adypt_set_noise_stats(adypt_ctx *c, int enabled)
{
	if(!c) return ADYPT_E_INVALID;
	if((enabled != 0) == (c->noise_stats != 0)) return ADYPT_OK;
	if(!enabled && c->ab.any_frozen()) return fail(c, ADYPT_E_STATE, "adypt_set_noise_stats: blocks are frozen at the noise target (adypt_trace_adaptive): reset first");
	if(enabled && c->spp != 0) return fail(c, ADYPT_E_STATE, "adypt_set_noise_stats: the moments start with the image: enable at 0 spp (after adypt_create, adypt_reset or adypt_trace_primary)");
	ENTER_DRAINED(c); // (the running-mean kernels enqueued so far have left the moments)
	if(!enabled)
	{
		c->noise_stats = 0;
		c->d_noise_moments.release(); c->d_noise_blocks.release(); c->d_noise_e.release();
		return ADYPT_OK;
	}
	if(c->n_local_px > 0)
	{
		const hipError_t e1 = c->d_noise_moments.alloc((size_t)c->n_local_px * sizeof(NoiseMoments));
		const hipError_t e2 = e1 == hipSuccess ? c->d_noise_blocks.alloc((size_t)c->n_local_blocks * sizeof(NoiseBlock)) : e1;
		if(e2 != hipSuccess)
		{
			c->d_noise_moments.release(); c->d_noise_blocks.release();
			(void)hipGetLastError();
			return fail(c, e2 == hipErrorOutOfMemory ? ADYPT_E_OOM : ADYPT_E_HIP, std::string("adypt_set_noise_stats: ") + hipGetErrorString(e2));
		}
	}
	c->noise_stats = 1;
	return ADYPT_OK;
}

int adypt_get_noise_stats(const adypt_ctx *c) { return c ? c->noise_stats : ADYPT_E_INVALID; }

}  // extern "C"

namespace {

// k_noise_blocks behind the pending running-mean kernels on the context's stream; the block results on the host when the call returns.
// per_pixel: the per-pixel noise is left in d_noise_e as well.  n_local_px > 0.
int query_noise_blocks(adypt_ctx *c, std::vector<NoiseBlock> *blocks, bool per_pixel)
{
	if(per_pixel && !c->d_noise_e) HIP_TRY(c, c->d_noise_e.alloc((size_t)c->n_local_px * sizeof(float))); // once: the size never changes
	// every owned block in the owned order, whatever is frozen: a frozen block at the frames it stopped at
	const dim3 grid((unsigned)c->n_local_blocks), block(256);
	const NoiseMoments *moments = c->d_noise_moments;
	const int32_t *owned = c->d_local_blocks, *no_count = nullptr;
	float *e_out = per_pixel ? c->d_noise_e.get() : nullptr;
	if(c->ab.any_frozen())
		hipLaunchKernelGGL(k_noise_blocks<true>, grid, block, 0, c->stream, moments, owned, c->blocks_x, c->width, c->height, c->spp, (const int32_t *)c->adaptive.frozen_at, c->d_noise_blocks.get(), e_out);
	else
		hipLaunchKernelGGL(k_noise_blocks<false>, grid, block, 0, c->stream, moments, owned, c->blocks_x, c->width, c->height, c->spp, no_count, c->d_noise_blocks.get(), e_out);
	HIP_TRY(c, hipGetLastError());
	blocks->resize((size_t)c->n_local_blocks);
	HIP_TRY(c, hipMemcpyAsync(blocks->data(), c->d_noise_blocks, blocks->size() * sizeof(NoiseBlock), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return ADYPT_OK;
}

// scatters an array of `per_px` floats per local pixel into the W x H image of the same
int read_local_floats(adypt_ctx *c, const float *device, int per_px, float *image)
{
	std::vector<float> local((size_t)c->n_local_px * per_px);
	HIP_TRY(c, hipMemcpyAsync(local.data(), device, local.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	for_each_local_pixel(c->local_blocks, c->width, c->height, [&](size_t L, int x, int y) {
		memcpy(image + ((size_t)y * c->width + x) * per_px, &local[L * per_px], sizeof(float) * per_px);
	});
	return ADYPT_OK;
}

}  // namespace

namespace adypt {
int ctx_read_blocks(adypt_ctx *c, std::vector<BlockState> *blocks)
{
	if(c->n_local_px == 0) return ADYPT_OK; // a shard that owns no block
	ENTER(c); // (not drained: the query is enqueued behind the frames)
	std::vector<NoiseBlock> found;
	TRY_CREATE(query_noise_blocks(c, &found, false));
	blocks->reserve(blocks->size() + found.size());
	for(size_t i = 0; i < found.size(); ++i)
		blocks->push_back(BlockState{c->local_blocks[i], found[i].sum, found[i].count, c->ab.spp_of(i, c->spp), c->ab.frozen_at[i] != 0});
	return ADYPT_OK;
}
}  // namespace adypt

extern "C" {

int adypt_get_noise(adypt_ctx *c, adypt_noise *out)
{
	if(!c || !out) return ADYPT_E_INVALID;
	TRY_CREATE(noise_ready(c, "adypt_get_noise", 2));
	memset(out, 0, sizeof(*out));
	out->spp = c->spp;
	std::vector<BlockState> blocks;
	TRY_CREATE(ctx_read_blocks(c, &blocks));
	const NoiseImage img = noise_of_image(blocks.data(), blocks.size(), c->n_image_px);
	out->mean_noise = img.mean_noise; out->worst_block = img.worst_block; out->worst_index = img.worst_index; out->pixels = c->n_image_px;
	return ADYPT_OK;
}

int adypt_read_noise(adypt_ctx *c, float *e)
{
	if(!c || !e) return ADYPT_E_INVALID;
	TRY_CREATE(noise_ready(c, "adypt_read_noise", 2));
	if(c->n_local_px == 0) return ADYPT_OK;
	ENTER(c);
	std::vector<NoiseBlock> blocks;
	TRY_CREATE(query_noise_blocks(c, &blocks, true));
	return read_local_floats(c, c->d_noise_e, 1, e);
}

int adypt_read_noise_moments(adypt_ctx *c, float *mean_m2)
{
	if(!c || !mean_m2) return ADYPT_E_INVALID;
	TRY_CREATE(noise_ready(c, "adypt_read_noise_moments", 0));
	if(c->n_local_px == 0) return ADYPT_OK;
	if(c->spp == 0) // nothing accumulated yet: the state of a cleared image
	{
		for_each_local_pixel(c->local_blocks, c->width, c->height, [&](size_t, int x, int y) { float *o = mean_m2 + ((size_t)y * c->width + x) * 2; o[0] = o[1] = 0.0f; });
		return ADYPT_OK;
	}
	ENTER(c);
	return read_local_floats(c, (const float *)c->d_noise_moments.get(), 2, mean_m2);
}

int64_t adypt_read_block_noise(adypt_ctx *c, int32_t *block_index, double *sum, uint32_t *count, int64_t capacity)
{
	if(!c || capacity < 0) return ADYPT_E_INVALID;
	TRY_CREATE(noise_ready(c, "adypt_read_block_noise", 2));
	const int64_t n = c->n_local_blocks;
	if(n == 0 || capacity < n) return n; // (the size alone: nothing is written)
	if(!block_index || !sum || !count) return ADYPT_E_INVALID;
	std::vector<BlockState> blocks;
	TRY_CREATE(ctx_read_blocks(c, &blocks));
	for(int64_t i = 0; i < n; ++i) { block_index[i] = blocks[(size_t)i].index; sum[i] = blocks[(size_t)i].sum; count[i] = blocks[(size_t)i].count; }
	return n;
}

int adypt_trace_until(adypt_ctx *c, double target, int min_spp, int max_spp, int check_every, adypt_noise *out)
{
	if(!c) return ADYPT_E_INVALID;
	TRY_CREATE(noise_ready(c, "adypt_trace_until", 0));
	std::string refused;
	const int r = trace_until("adypt_trace_until", &refused, target, min_spp, max_spp, check_every, out, [c] { return c->spp; }, [c](int n) { return adypt_trace_spp(c, n); },
	                          [c](adypt_noise *o) { return adypt_get_noise(c, o); });
	return refused.empty() ? r : fail(c, r, refused);
}

int64_t adypt_read_block_spp(adypt_ctx *c, int32_t *block_index, int32_t *spp, int64_t capacity)
{
	if(!c || capacity < 0) return ADYPT_E_INVALID;
	const int64_t n = c->n_local_blocks;
	if(n == 0 || capacity < n) return n; // (the size alone: nothing is written)
	if(!block_index || !spp) return ADYPT_E_INVALID;
	for(int64_t i = 0; i < n; ++i) { block_index[i] = c->local_blocks[(size_t)i]; spp[i] = c->ab.spp_of((size_t)i, c->spp); }
	return n;
}

int adypt_trace_adaptive(adypt_ctx *c, double target, int min_spp, int max_spp, int check_every, adypt_adaptive *out)
{
	if(!c) return ADYPT_E_INVALID;
	TRY_CREATE(ctx_adaptive_ready(c, "adypt_trace_adaptive"));
	std::string refused;
	const int r = trace_adaptive("adypt_trace_adaptive", &refused, target, min_spp, max_spp, check_every, out, [c] { return c->spp; }, [c](int n) { return adypt_trace_spp(c, n); },
	                             [c](std::vector<BlockState> *blocks) { blocks->clear(); return ctx_read_blocks(c, blocks); },
	                             [c](const std::vector<int32_t> &stop, int spp) { return freeze_blocks(c, stop.data(), stop.size(), spp); });
	return refused.empty() ? r : fail(c, r, refused);
}

static int trace_rays_impl(adypt_ctx *c, const float *rays, int64_t n, adypt_hit *hits, int with_stats, bool any_hit)
{
	if(!c || n < 0 || (n > 0 && (!rays || !hits))) return ADYPT_E_INVALID;
	if(!c->queues_ok) return fail(c, ADYPT_E_STATE, "adypt_trace_rays: the context lost its ray queues (failed adypt_set_frames_in_flight)");
	ENTER(c);
	drop_rolling(c); // (a frame started ahead works in a window of the queues this call is about to fill)
	if(!c->pt_started) TRY_CREATE(apply_params(c));
	if(with_stats) TRY_CREATE(ensure_ray_stats(c));
	std::vector<float4> o, d, h;
	std::vector<RayStats> rs;
	for(int64_t done = 0; done < n;)
	{
		const int64_t m = std::min<int64_t>(n - done, c->capacity);
		o.resize((size_t)m); d.resize((size_t)m); h.resize((size_t)m);
		for(int64_t i = 0; i < m; ++i)
		{
			const float *r = rays + (size_t)(done + i) * 8;
			o[(size_t)i] = make_float4(r[0], r[1], r[2], r[3]);
			d[(size_t)i] = make_float4(r[4], r[5], r[6], 0.0f);
		}
		// the batch is cut into kNumSegments consecutive pieces, piece s occupying the head of queue segment s
		clear_counters(c, c->d_counters, 1, c->stream);
		const int64_t piece = (m + kNumSegments - 1) / kNumSegments; // <= seg_cap because m <= capacity
		uint32_t counts[kNumSegments * kCursorStride] = {0};
		if(with_stats) rs.resize((size_t)m);
		for(int s = 0; s < kNumSegments; ++s)
		{
			const int64_t b0 = std::min<int64_t>(piece * s, m), n_s = std::min<int64_t>(piece, m - b0);
			counts[s * kCursorStride] = (uint32_t)n_s;
			if(n_s <= 0) continue;
			const size_t off = (size_t)s * c->seg_cap;
			HIP_TRY(c, hipMemcpyAsync(c->q.o[0] + off, o.data() + b0, (size_t)n_s * sizeof(float4), hipMemcpyHostToDevice, c->stream));
			HIP_TRY(c, hipMemcpyAsync(c->q.d[0] + off, d.data() + b0, (size_t)n_s * sizeof(float4), hipMemcpyHostToDevice, c->stream));
		}
		HIP_TRY(c, hipMemcpyAsync(c->d_counters->count[0], counts, sizeof(counts), hipMemcpyHostToDevice, c->stream));
		TRY_CREATE(launch_trace(c, c->pipes[0], full_window(c), 0, c->d_counters->count[0], c->d_counters->cursor[0], c->params.stack_size, with_stats != 0, with_stats ? c->q.ray_stats : nullptr, any_hit));
		for(int s = 0; s < kNumSegments; ++s)
		{
			const int64_t b0 = std::min<int64_t>(piece * s, m), n_s = std::min<int64_t>(piece, m - b0);
			if(n_s <= 0) continue;
			const size_t off = (size_t)s * c->seg_cap;
			HIP_TRY(c, hipMemcpyAsync(h.data() + b0, c->q.hit + off, (size_t)n_s * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
			if(with_stats) HIP_TRY(c, hipMemcpyAsync(rs.data() + b0, c->q.ray_stats + off, (size_t)n_s * sizeof(RayStats), hipMemcpyDeviceToHost, c->stream));
		}
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		for(int64_t i = 0; i < m; ++i)
		{
			adypt_hit &out = hits[done + i];
			memcpy(&out.tri_id, &h[(size_t)i].x, 4);
			out.u = h[(size_t)i].y; out.v = h[(size_t)i].z; out.t = h[(size_t)i].w;
			if(with_stats)
			{
				const RayStats &s = rs[(size_t)i];
				out.ref_idx = s.ref_idx; out.nodes = s.nodes; out.tris = s.tris; out.hash = s.hash; out.max_depth = s.max_depth;
			}
			else { out.ref_idx = out.tri_id == -1 ? -1 : 0; out.nodes = out.tris = out.hash = out.max_depth = 0; }
		}
		done += m;
	}
	harvest_events(c);
	return ADYPT_OK; // stack overflows of arbitrary batches are reported per ray (max_depth = 0xffffffff) and in the stats
}

int adypt_trace_rays(adypt_ctx *c, const float *rays, int64_t n, adypt_hit *hits, int with_stats)
{
	return trace_rays_impl(c, rays, n, hits, with_stats, false);
}

int adypt_trace_rays_any(adypt_ctx *c, const float *rays, int64_t n, adypt_hit *hits, int with_stats)
{
	return trace_rays_impl(c, rays, n, hits, with_stats, true);
}

int adypt_get_stats(adypt_ctx *c, adypt_stats *out)
{
	if(!c || !out) return ADYPT_E_INVALID;
	DeviceStats st;
	TRY_CREATE(read_device_stats(c, &st));
	harvest_events(c);
	out->rays = st.rays; out->nodes_visited = st.nodes; out->tris_tested = st.tris; out->hits = st.hits; out->shaded = st.shaded;
	out->stack_overflows = st.overflows; out->bad_materials = st.bad_materials; out->max_stack = st.max_stack;
	out->trace_launches = c->trace_launches; out->trace_ms = c->trace_ms; out->shade_ms = c->shade_ms;
	out->path_ms = c->path_ms; out->path_launches = c->path_launches; out->audit_errors = (uint32_t)std::min<unsigned long long>(st.audit_errors, 0xffffffffull);
	out->path_rays = st.path_rays; out->path_nodes = st.path_nodes; out->path_tris = st.path_tris; out->path_hits = st.path_hits; out->path_shaded = st.path_shaded;
	return ADYPT_OK;
}

int adypt_get_shader_clock(adypt_ctx *c, uint64_t out[2])
{
	if(!c || !out) return ADYPT_E_INVALID;
	DeviceStats st;
	TRY_CREATE(read_device_stats(c, &st));
	out[0] = st.clock_cycles; out[1] = st.clock_ticks;
	return ADYPT_OK;
}

int adypt_get_wave_profile(adypt_ctx *c, uint64_t out[8])
{
	if(!c || !out) return ADYPT_E_INVALID;
	DeviceStats st;
	TRY_CREATE(read_device_stats(c, &st));
	for(int i = 0; i < 8; ++i) out[i] = st.wave_profile[i];
	return ADYPT_OK;
}

int adypt_read_root_card(adypt_ctx *c, void *card_out)
{
	if(!c || !card_out) return ADYPT_E_INVALID;
	ENTER_DRAINED(c);
	if(!c->d_root_card) return fail(c, ADYPT_E_STATE, "adypt_read_root_card: the context has no root card");
	HIP_TRY(c, hipMemcpy(card_out, c->d_root_card, sizeof(RootCard), hipMemcpyDeviceToHost));
	return ADYPT_OK;
}

int adypt_reset_stats(adypt_ctx *c)
{
	if(!c) return ADYPT_E_INVALID;
	ENTER_DRAINED(c);
	harvest_events(c);
	// on the context's own stream: a legacy-stream hipMemset is not ordered against a non-blocking stream
	HIP_TRY(c, hipMemsetAsync(c->d_stats, 0, offsetof(DeviceStats, host_overflow), c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	*c->h_overflow = 0u;
	c->trace_ms = c->shade_ms = c->path_ms = 0; c->trace_launches = c->path_launches = 0;
	return ADYPT_OK;
}

int64_t adypt_local_pixel_count(const adypt_ctx *c) { return c ? c->n_local_px : ADYPT_E_INVALID; }

int adypt_copy_local_radiance(adypt_ctx *c, void *dst, int64_t capacity_float4)
{
	if(!c || !dst || capacity_float4 < c->n_local_px) return ADYPT_E_INVALID;
	ENTER(c); // (not drained, as adypt_read_display: the copy is enqueued behind the frames)
	HIP_TRY(c, hipMemcpyAsync(dst, c->d_accum, (size_t)c->n_local_px * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
	if(capacity_float4 > c->n_local_px)
		HIP_TRY(c, hipMemsetAsync((char *)dst + (size_t)c->n_local_px * sizeof(float4), 0, (size_t)(capacity_float4 - c->n_local_px) * sizeof(float4), c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return ADYPT_OK;
}

int adypt_assemble_radiance(adypt_ctx *c, const void *gathered, int64_t stride_float4, void *rgb_device)
{
	if(!c || !gathered || !rgb_device || stride_float4 < 0) return ADYPT_E_INVALID;
	ENTER(c);
	if(!c->d_all_blocks)
	{
		// block lists of every rank of the shard, back to back (uploaded once)
		std::vector<int32_t> all;
		c->all_blocks_offset.assign(1, 0);
		for(int r = 0; r < c->nranks; ++r)
		{
			const std::vector<int32_t> b = owned_blocks(c->width, c->height, r, c->nranks);
			all.insert(all.end(), b.begin(), b.end());
			c->all_blocks_offset.push_back((int64_t)all.size());
		}
		TRY_CREATE(upload(c, &c->d_all_blocks, all.data(), all.size()));
	}
	for(int r = 0; r < c->nranks; ++r)
	{
		const int64_t n_blocks = c->all_blocks_offset[(size_t)r + 1] - c->all_blocks_offset[(size_t)r];
		const int n_px = (int)(n_blocks * kBlockPixels);
		if(n_px == 0) continue;
		if(stride_float4 < n_px) return fail(c, ADYPT_E_INVALID, "adypt_assemble_radiance: stride smaller than a rank's buffer");
		hipLaunchKernelGGL(k_untile, dim3((n_px + 255) / 256), dim3(256), 0, c->stream, (const float4 *)gathered + (size_t)r * (size_t)stride_float4,
						   (const int32_t *)c->d_all_blocks + c->all_blocks_offset[(size_t)r], n_px, c->blocks_x, c->width, c->height, (float *)rgb_device);
	}
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	return ADYPT_OK;
}

int adypt_local_radiance_device(adypt_ctx *c, void **dptr)
{
	if(!c || !dptr) return ADYPT_E_INVALID;
	*dptr = c->d_accum;
	return ADYPT_OK;
}

}  // extern "C"
