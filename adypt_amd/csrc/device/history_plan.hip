// History-aware sampling (include/adypt_hip.h adypt_plan_by_history ...; the definition: history_reach.hpp).  A translation unit of its own: nothing
// here is part of the tracer's or the denoiser's code object.  What runs, on the context's stream, before the first sample of a pose:
//     guide capture     three launches of the viewer instance of k_trace_camera over the owned blocks at 0 spp (tracer.hip ctx_capture_guides), into
//                       the denoiser's block-major scratch (denoise_internal.hpp denoise_plan_inputs), which the next denoise call captures again
//     k_history_reach   one workgroup per 32 x 32 block: the reach of every local pixel (history_reach.hpp) and the block's 65 bins
// then the bins come to the host (260 B per block), where plan_block gives every block its sample count; adypt_trace_by_history follows the plan
// through trace_plan, over the context's own adypt_trace_spp and ctx_freeze_blocks.  Several devices: denoise_plan_inputs_multi brings every device's
// guides to the first one as adypt_multi_denoise does, the kernel runs there over all blocks (the history lives there), and every device freezes its
// own blocks through the same trace_plan.
#include "ctx_unit.hpp"
#include "tile_layout.hpp"
#include "history_reach.hpp"
#include "denoise_internal.hpp"
#include "../../../include/adypt_hip.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace adypt;

namespace {

constexpr int kReachThreads = 256;                              // the workgroup: a block's 1024 local pixels, 4 per thread
constexpr int kReachPerThread = kBlockPixels / kReachThreads;
constexpr int kReachTriVecs = 5;                                // the first 80 bytes of a record, as the snapshot keeps them (words 0..17 are read)
static_assert(kReachTriVecs * 4 >= kTemporalTriWords, "the words temporal_previous_point reads");

struct ReachHistory {
	const float4 *a, *b, *c, *d;
	__device__ __forceinline__ static Dn4 load(const float4 *p, int i) { const float4 v = p[i]; return Dn4{v.x, v.y, v.z, v.w}; }
	__device__ __forceinline__ Dn4 h0(int i) const { return load(a, i); }
	__device__ __forceinline__ Dn4 h1(int i) const { return load(b, i); }
	__device__ __forceinline__ Dn4 h2(int i) const { return load(c, i); }
	__device__ __forceinline__ Dn4 ha(int i) const { return load(d, i); }
};
struct ReachGuides { const float4 *albedo, *normal, *position, *hits; const int32_t *blocks; };        // block-major, as ctx_capture_guides fills them
struct ReachSnapshot { const float4 *snapshot, *records; int64_t n_known; int tri_float4; };            // MOTION only

__device__ __forceinline__ void reach_unpack_tri(const float4 *__restrict__ q, float w[kReachTriVecs * 4])
{
#pragma unroll
	for(int k = 0; k < kReachTriVecs; ++k)
	{
		const float4 v = q[k];
		w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
	}
}

// Workgroup b takes block b of the list; thread t its local pixels t, t + 256, t + 512, t + 768 — a wave reads one 8 x 8 tile of 64 consecutive
// local pixels at a time, 16 B each: the local-pixel layout of k_denoise_prepare.  Per hit pixel it reads the four guides (64 B) and up to four taps x
// 64 B of the history's row-major images (neighbouring pixels share them); MOTION: where the hit triangle lies inside the snapshot, 80 B of it and 80 B
// of the record as it is now, inline (k_motion_gather's fetch; no XP / XN is written).  The words history_reach is given are the ones
// denoise_prepare_pixel<false> would write to X1, X2 and XA for the pixel: the hit flag from hits.x != -1, the albedo as captured.  Writes the reach of
// every local pixel (4 B; 0 outside the image) and the block's 65 bins, counted in LDS — integers: the order of the additions does not matter — and
// written with plain stores by the workgroup that owns the block: no global atomic.  Every array of a lane is indexed by constants after unrolling.
template <bool MOTION>
__global__ __launch_bounds__(kReachThreads) void k_history_reach(ReachGuides g, int n_blocks, int blocks_x, int width, int height, ReachHistory hist, int have, TemporalCamera cam,
                                                                  float history_cap, ReachSnapshot snap, float *__restrict__ reach, uint32_t *__restrict__ bins)
{
	__shared__ uint32_t count[kReachBins];
	const int b = blockIdx.x;
	if(b >= n_blocks) return; // (uniform over the workgroup)
	if(threadIdx.x < kReachBins) count[threadIdx.x] = 0u;
	__syncthreads();
	const int blk = g.blocks[b];
#pragma unroll 1
	for(int k = 0; k < kReachPerThread; ++k)
	{
		const int in = k * kReachThreads + (int)threadIdx.x;
		const size_t L = (size_t)b * kBlockPixels + in;
		int x, y;
		block_pixel_xy(blk, in, blocks_x, &x, &y);
		float r = 0.0f;
		if(x < width && y < height)
		{
			const float4 hq = g.hits[L];
			const int32_t tri = __float_as_int(hq.x);
			const bool hit = tri != -1;
			if(hit && have != 0)
			{
				const float4 a = g.albedo[L], n = g.normal[L], q = g.position[L];
				const Dn4 c1{n.x, n.y, n.z, 1.0f}, c2{q.x, q.y, q.z, 0.0f}, ca{a.x, a.y, a.z, 0.0f};
				if(MOTION)
				{
					const bool known = tri >= 0 && (int64_t)tri < snap.n_known;
					float prev[kReachTriVecs * 4] = {}, cur[kReachTriVecs * 4] = {};
					if(known)
					{
						reach_unpack_tri(snap.snapshot + (size_t)tri * kReachTriVecs, prev);
						reach_unpack_tri(snap.records + (size_t)tri * (size_t)snap.tri_float4, cur);
					}
					const TemporalPrevious p = temporal_previous_point(prev, cur, known, hq.y, hq.z, c1, c2);
					r = history_reach_motion(hist, true, cam, width, height, c1, ca, history_cap, p.xp, p.xn);
				}
				else r = history_reach_still(hist, true, cam, width, height, c1, c2, ca, history_cap);
			}
			if(hit) atomicAdd(&count[reach_bin(r)], 1u);
		}
		reach[L] = r;
	}
	__syncthreads();
	if(threadIdx.x < kReachBins) bins[(size_t)b * kReachBins + threadIdx.x] = count[threadIdx.x];
}

// What the unit keeps per context (ctx_attachment kAttachHistoryPlan): the reach image and the bins on the device, 4 B per local pixel + 260 B per
// block, allocated at the first plan; and the last plan on the host, in the order of the block list it was made over.
struct PlanState {
	Buffer<float> reach;
	Buffer<uint32_t> bins;
	StageTimer<3> timer;                 // start, behind the capture, behind the reach kernel
	bool valid = false;                  // a plan ran to its end: the read-outs answer
	int width = 0, height = 0;
	std::vector<int32_t> block_index;    // the block list of the last plan (one device: the owned blocks, ascending; several: rank order)
	std::vector<uint32_t> host_bins;     // 65 per block of that list
	std::vector<int32_t> want;           // per block of that list
};

adypt_history_plan_params plan_params(const adypt_history_plan_params *p)
{
	return p ? *p : adypt_history_plan_params{16, 2, 64, 4, kPlanDefaultTolerance, kTemporalDefaultCap, 0, 0};
}
std::string refusal(const char *fn, const adypt_history_plan_params &p)
{
	if(plan_args_valid(p.target, p.min_spp, p.max_spp, p.step, p.tolerance_permille, p.history_cap)) return {};
	return std::string(fn) + ": needs 1 <= target <= " + std::to_string(kPlanMaxTarget) + ", 2 <= min_spp <= max_spp, step >= 1, 0 <= tolerance_permille <= 999 and a history_cap that is a positive finite number";
}

// pixels of image block `blk` that lie inside the image
int64_t block_image_px(int blk, int width, int height)
{
	const int blocks_x = (width + kBlockDim - 1) / kBlockDim;
	return (int64_t)std::min(kBlockDim, width - (blk % blocks_x) * kBlockDim) * (int64_t)std::min(kBlockDim, height - (blk / blocks_x) * kBlockDim);
}

// the places of the block list in ascending order of block index
std::vector<size_t> ascending(const std::vector<int32_t> &block_index)
{
	std::vector<size_t> order(block_index.size());
	for(size_t i = 0; i < order.size(); ++i) order[i] = i;
	std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return block_index[a] < block_index[b]; });
	return order;
}

// The reach kernel over the set `in` on context c (its device current), the bins to the host, the plan: s->want, *info.  `in` comes with the capture
// enqueued (mark 1 stands behind it).
int plan_on(adypt_ctx *c, PlanState *s, const PlanInputs &in, const adypt_history_plan_params &p, adypt_history_plan *info)
{
	const CtxInfo i = ctx_info(c);
	const size_t n_blocks = (size_t)in.n_blocks;
	s->valid = false;
	s->width = i.width; s->height = i.height;
	CTX_TRY(c, at_least(s->reach, n_blocks * kBlockPixels));
	CTX_TRY(c, at_least(s->bins, n_blocks * kReachBins));
	CTX_TRY(c, s->timer.mark(1, i.stream));
	s->block_index = in.block_index;
	s->host_bins.assign(n_blocks * kReachBins, 0u);
	if(n_blocks > 0)
	{
		const CtxScene sc = ctx_scene(c);
		const ReachGuides g{in.albedo, in.normal, in.position, in.hits, in.blocks};
		const ReachHistory hist{in.h0, in.h1, in.h2, in.ha};
		const ReachSnapshot snap{in.snapshot, (const float4 *)sc.triangles, in.snapshot ? in.known_tris : 0, sc.tri_float4};
		const int blocks_x = (i.width + kBlockDim - 1) / kBlockDim;
		hipLaunchKernelGGL(p.follow_motion ? k_history_reach<true> : k_history_reach<false>, dim3((unsigned)n_blocks), dim3(kReachThreads), 0, i.stream, g, (int)n_blocks, blocks_x, i.width, i.height,
		                   hist, in.have, in.camera, p.history_cap, snap, s->reach.get(), s->bins.get());
		CTX_TRY(c, hipGetLastError());
	}
	CTX_TRY(c, s->timer.mark(2, i.stream));
	if(n_blocks > 0) CTX_TRY(c, hipMemcpyAsync(s->host_bins.data(), s->bins.get(), s->host_bins.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	s->want.resize(n_blocks);
	adypt_history_plan out;
	memset(&out, 0, sizeof(out));
	out.blocks = (int32_t)n_blocks;
	uint64_t floors = 0;
	for(size_t b = 0; b < n_blocks; ++b)
	{
		const uint32_t *bins = s->host_bins.data() + b * kReachBins;
		const int want = plan_block(bins, p.target, p.min_spp, p.max_spp, p.step, p.tolerance_permille);
		s->want[b] = want;
		out.want_min = b == 0 ? want : std::min(out.want_min, want);
		out.want_max = b == 0 ? want : std::max(out.want_max, want);
		const int64_t px = block_image_px(in.block_index[b], i.width, i.height);
		out.pixels += px;
		out.pixel_samples += px * want;
		for(int k = 1; k < kReachBins; ++k) { out.pixels_with_history += bins[k]; floors += (uint64_t)bins[k] * (uint64_t)k; }
	}
	out.mean_reach = out.pixels > 0 ? (double)floors / (double)out.pixels : 0.0;
	float ms[2] = {0.0f, 0.0f};
	(void)s->timer.read(ms, 2, 2, false);
	out.capture_ms = ms[0]; out.reach_ms = ms[1];
	out.device_bytes = (int64_t)(s->reach.bytes() + s->bins.bytes());
	s->valid = true;
	if(info) *info = out;
	return ADYPT_OK;
}

PlanState *plan_state(adypt_ctx *c) { return ctx_state<PlanState>(c, kAttachHistoryPlan); }
PlanState *finished_plan(adypt_ctx *c, const char *fn)
{
	PlanState *s = ctx_state_if_any<PlanState>(c, kAttachHistoryPlan);
	if(s && s->valid) return s;
	ctx_set_error(c, std::string(fn) + ": no plan has been made yet (adypt_plan_by_history)");
	return nullptr;
}

// (block, want) of the last plan
std::vector<std::pair<int32_t, int32_t>> wants_of(const PlanState *s)
{
	std::vector<std::pair<int32_t, int32_t>> w;
	for(size_t b = 0; b < s->want.size(); ++b) w.emplace_back(s->block_index[b], s->want[b]);
	return w;
}

// the plan of one context
int plan_context(adypt_ctx *c, const char *fn, const adypt_history_plan_params *params, adypt_history_plan *info)
{
	if(!c) return ADYPT_E_INVALID;
	const adypt_history_plan_params p = plan_params(params);
	const std::string refused = refusal(fn, p);
	if(!refused.empty()) return ctx_fail(c, ADYPT_E_INVALID, refused);
	const CtxInfo i = ctx_info(c);
	if(i.nranks != 1) return ctx_fail(c, ADYPT_E_STATE, std::string(fn) + ": the context is a tile shard (tile_nranks > 1): the history is the whole image's (adypt_multi_plan_by_history)");
	CTX_STEP(ctx_plan_ready(c, fn));
	CTX_TRY(c, hipSetDevice(i.device));
	PlanState *s = plan_state(c);
	s->valid = false;
	CTX_TRY(c, s->timer.mark(0, i.stream));
	PlanInputs in;
	CTX_STEP(denoise_plan_inputs(c, fn, p.moments != 0, &in));
	return plan_on(c, s, in, p, info);
}

int trace_context(adypt_ctx *c, const char *fn, const adypt_history_plan_params *params, adypt_history_plan *info)
{
	adypt_history_plan out;
	CTX_STEP(plan_context(c, fn, params, &out));
	CTX_STEP(trace_plan(wants_of(plan_state(c)), [c] { return ctx_spp(c); }, [c](int n) { return adypt_trace_spp(c, n); },
	                    [c](const std::vector<int32_t> &stop, int spp) { return ctx_freeze_blocks(c, stop.data(), stop.size(), spp); }));
	out.spp = ctx_spp(c);
	if(info) *info = out;
	return ADYPT_OK;
}

int read_reach(adypt_ctx *c, const char *fn, float *reach)
{
	PlanState *s = finished_plan(c, fn);
	if(!s) return ADYPT_E_STATE;
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	std::vector<float> local(s->block_index.size() * kBlockPixels);
	if(!local.empty()) CTX_TRY(c, hipMemcpyAsync(local.data(), s->reach.get(), local.size() * sizeof(float), hipMemcpyDeviceToHost, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	for_each_local_pixel(s->block_index, s->width, s->height, [&](size_t L, int x, int y) { reach[(size_t)y * s->width + x] = local[L]; });
	return ADYPT_OK;
}

int64_t read_plan(adypt_ctx *c, const char *fn, int32_t *block_index, int32_t *want, uint32_t *bins, int64_t capacity)
{
	if(capacity < 0) return ADYPT_E_INVALID;
	PlanState *s = finished_plan(c, fn);
	if(!s) return ADYPT_E_STATE;
	const int64_t n = (int64_t)s->block_index.size();
	if(!block_index || (!want && !bins) || capacity < n) return n; // (the size alone: nothing is written)
	const std::vector<size_t> order = ascending(s->block_index);
	for(int64_t k = 0; k < n; ++k)
	{
		const size_t b = order[(size_t)k];
		block_index[k] = s->block_index[b];
		if(want) want[k] = s->want[b];
		if(bins) memcpy(bins + (size_t)k * kReachBins, s->host_bins.data() + b * kReachBins, kReachBins * sizeof(uint32_t));
	}
	return n;
}

// ---- one process, N devices ----
int multi_fail(adypt_multi *m, int code, const std::string &msg) { multi_set_error(m, msg); return code; }

int plan_multi(adypt_multi *m, const char *fn, const adypt_history_plan_params *params, adypt_history_plan *info)
{
	const int n_dev = adypt_multi_device_count(m);
	if(n_dev < 1) return ADYPT_E_INVALID;
	if(n_dev == 1) return multi_each(m, [&](adypt_ctx *c) { return plan_context(c, fn, params, info); });
	const adypt_history_plan_params p = plan_params(params);
	const std::string refused = refusal(fn, p);
	if(!refused.empty()) return multi_fail(m, ADYPT_E_INVALID, refused);
	CTX_STEP(multi_each(m, [fn](adypt_ctx *c) { return ctx_plan_ready(c, fn); }));
	adypt_ctx *root = adypt_multi_context(m, 0);
	auto steps = [&]() -> int {
		adypt_ctx *c = root;
		const CtxInfo ri = ctx_info(c);
		CTX_TRY(c, hipSetDevice(ri.device));
		PlanState *s = plan_state(c);
		s->valid = false;
		CTX_TRY(c, s->timer.mark(0, ri.stream));
		return ADYPT_OK;
	};
	int r = steps();
	if(r != ADYPT_OK) return multi_fail(m, r, adypt_last_error(root));
	PlanInputs in;
	CTX_STEP(denoise_plan_inputs_multi(m, fn, p.moments != 0, &in)); // (the first device is current again)
	r = plan_on(root, plan_state(root), in, p, info);
	return r == ADYPT_OK ? r : multi_fail(m, r, adypt_last_error(root));
}

int trace_multi(adypt_multi *m, const char *fn, const adypt_history_plan_params *params, adypt_history_plan *info)
{
	const int n_dev = adypt_multi_device_count(m);
	if(n_dev < 1) return ADYPT_E_INVALID;
	if(n_dev == 1) return multi_each(m, [&](adypt_ctx *c) { return trace_context(c, fn, params, info); });
	adypt_history_plan out;
	CTX_STEP(plan_multi(m, fn, params, &out));
	CTX_STEP(trace_plan(wants_of(plan_state(adypt_multi_context(m, 0))), [m] { return adypt_multi_get_spp(m); }, [m](int n) { return adypt_multi_trace_spp(m, n); },
	                    [m](const std::vector<int32_t> &stop, int spp) { return multi_each(m, [&](adypt_ctx *c) { return ctx_freeze_blocks(c, stop.data(), stop.size(), spp); }); }));
	out.spp = adypt_multi_get_spp(m);
	if(info) *info = out;
	return ADYPT_OK;
}

// a read-out on the first device's context, its error becoming the handle's
template <class F> auto on_root(adypt_multi *m, F f) -> decltype(f((adypt_ctx *)nullptr))
{
	if(adypt_multi_device_count(m) < 1) return ADYPT_E_INVALID;
	adypt_ctx *root = adypt_multi_context(m, 0);
	const auto r = f(root);
	if(r < 0) multi_set_error(m, adypt_last_error(root));
	return r;
}

}  // namespace

extern "C" {

int adypt_plan_by_history(adypt_ctx *c, const adypt_history_plan_params *params, adypt_history_plan *info) { return plan_context(c, "adypt_plan_by_history", params, info); }

int adypt_trace_by_history(adypt_ctx *c, const adypt_history_plan_params *params, adypt_history_plan *info) { return c ? trace_context(c, "adypt_trace_by_history", params, info) : ADYPT_E_INVALID; }

int adypt_read_history_reach(adypt_ctx *c, float *reach) { return c && reach ? read_reach(c, "adypt_read_history_reach", reach) : ADYPT_E_INVALID; }

int64_t adypt_read_sample_plan(adypt_ctx *c, int32_t *block_index, int32_t *want, int64_t capacity)
{
	return c ? read_plan(c, "adypt_read_sample_plan", want ? block_index : nullptr, want, nullptr, capacity) : ADYPT_E_INVALID;
}

int64_t adypt_read_history_bins(adypt_ctx *c, int32_t *block_index, uint32_t *bins, int64_t capacity)
{
	return c ? read_plan(c, "adypt_read_history_bins", bins ? block_index : nullptr, nullptr, bins, capacity) : ADYPT_E_INVALID;
}

int adypt_multi_plan_by_history(adypt_multi *m, const adypt_history_plan_params *params, adypt_history_plan *info) { return plan_multi(m, "adypt_multi_plan_by_history", params, info); }

int adypt_multi_trace_by_history(adypt_multi *m, const adypt_history_plan_params *params, adypt_history_plan *info) { return trace_multi(m, "adypt_multi_trace_by_history", params, info); }

int adypt_multi_read_history_reach(adypt_multi *m, float *reach)
{
	return reach ? on_root(m, [=](adypt_ctx *c) { return read_reach(c, "adypt_multi_read_history_reach", reach); }) : ADYPT_E_INVALID;
}

int64_t adypt_multi_read_sample_plan(adypt_multi *m, int32_t *block_index, int32_t *want, int64_t capacity)
{
	return on_root(m, [=](adypt_ctx *c) { return read_plan(c, "adypt_multi_read_sample_plan", want ? block_index : nullptr, want, nullptr, capacity); });
}

int64_t adypt_multi_read_history_bins(adypt_multi *m, int32_t *block_index, uint32_t *bins, int64_t capacity)
{
	return on_root(m, [=](adypt_ctx *c) { return read_plan(c, "adypt_multi_read_history_bins", bins ? block_index : nullptr, nullptr, bins, capacity); });
}

}  // extern "C"
