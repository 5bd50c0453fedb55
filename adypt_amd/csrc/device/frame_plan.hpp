// Which kernels the next wavefront pass of adypt_trace_spp_async launches — decided here, once, from plain numbers; frame_schedule.hpp enqueues
// what the plan says.  No HIP and no adypt_ctx: tests/test_frame_plan.py compiles this header with g++ and checks plan_pass over a grid of inputs.
//
// The pipelines a pass can take:
//   one-launch        k_shade_first (camera rays + bounce 0 from the cached primary hits) -> k_path (every later bounce, and the sun-visibility
//                     queries of the escaped paths among its rays) -> k_resolve.  One chain only; a single frame takes it as a ROLLING frame
//                     (frame k + 1 is enqueued under the end of frame k's k_path: frame_schedule.hpp, trace_rolling_frame)
//   launch-per-bounce [k_trace -> k_shade (-> any-hit k_trace of the sun-visibility query queue -> k_shadow_resolve)] per bounce, on 1-4 sub-batch
//                     chains ("pipes"); bounce 0 is k_shade_first (ADYPT_FIRST_FUSED=0 or a lone frame: k_gen_primary -> k_trace -> k_shade)
#pragma once
#include "path_limits.hpp"

#include <algorithm>
#include <cstdint>

namespace adypt {

constexpr int kMaxPipes = 4;           // sub-batches of a batch that run as concurrent chains (adypt_set_pipeline)

struct PlanInput {
	int spp, remaining;                // frames applied to the image so far / still asked for by the call (> 0)
	int lookahead, frames_in_flight, tmp_lifetime, max_bounce, pipeline;
	int single_fused, first_fused, fused_bounces, sun_visibility; // the tunables (tunables.hpp) and adypt_set_sun_visibility
	int64_t n_local_px;                // > 0: a shard that owns no block never gets here
	int noise_stats = 0;               // adypt_set_noise_stats: every finished sample is parked and applied by the running-mean kernel, which keeps the moments
	int cache_stale = 0;               // adaptive sampling changed the block set since the cache image was written: the pass-local pixel order is another (active_blocks.hpp)
};

struct PassPlan {
	enum Kind { Rolling, Batch } kind;
	int m, hand_out;                         // frames [spp, spp + m) are traced by the pass; the first hand_out go into the image now, the others stay parked
	int first_retrace, n_retrace, n_groups;  // frames with frame % tmpLifetime == 0 re-trace their primary rays: batch index of the first, how many, tmpLifetime groups spanned
	bool stale_retrace;                      // the pass starts inside a tmpLifetime group whose cached hits are stale: its first frame stands in for the group's re-tracing frame
	bool as_batch;                           // finished samples are parked and applied by k_resolve (false: the lone launch-per-bounce frame accumulates by itself, unless the noise statistics are on)
	bool use_cache;                          // bounce 0 starts from the cached primary hits (false: that lone frame re-traces, its k_gen_primary makes camera rays)
	bool fused_first, fused_bounces;         // bounce 0 is k_shade_first | the bounces after it are one k_path launch
	bool sun_query, sun_queue;               // sun visibility on: the queries ride in k_shade_first + k_path | go through the query queue after every k_shade
	int n_pipes, frames_of_pipe[kMaxPipes];
};

// A pass of `frames` frames on `n_pipes` chains may take the one-launch pipeline: the path word has 26 bits for the path id, and the sun-visibility
// query rides in k_path as bounce index kPwShadow = 31 — with 32 bounces configured the launch-per-bounce pipeline keeps it
inline bool one_launch_ok(const PlanInput &in, int frames, int n_pipes)
{
	const bool sun_ok = !in.sun_visibility || in.max_bounce <= (int)kPwShadow;
	return n_pipes == 1 && in.first_fused && in.fused_bounces && sun_ok && (int64_t)frames * in.n_local_px <= kPathMaxPaths;
}

inline PassPlan plan_pass(const PlanInput &in)
{
	PassPlan p{};
	const int life = std::max(1, in.tmp_lifetime);
	// Batch = up to frames_in_flight consecutive frames traced as ONE wavefront (frames are independent samples; the running mean is applied
	// afterwards in frame order, so the result is bit-identical to frame-by-frame).  With look-ahead on, a call for fewer frames than fit in a pass
	// (Instance::Update asks for ONE, src/Instance.cpp:44-57) still traces a full pass: the frames beyond the ones asked for are finished early and
	// parked; later calls hand them out one running-mean step at a time.
	p.m = in.lookahead ? in.frames_in_flight : std::min(in.remaining, in.frames_in_flight);
	p.hand_out = std::min(in.remaining, p.m);
	// A batch may span several tmpLifetime groups: its re-tracing frames run first, as one primary-only pass, and park their hits in the cache image of their group
	p.first_retrace = (life - in.spp % life) % life;
	p.n_retrace = p.first_retrace < p.m ? (p.m - 1 - p.first_retrace) / life + 1 : 0;
	p.n_groups = (in.spp + p.m - 1) / life - in.spp / life + 1;
	// A stale cache image: the camera rays of the group the pass starts in are traced again.  The primary hit is a function of the pixel and the group
	// alone (shade.hpp frame_group, sub_idx), so batch frame 0 gives the bits the group's own re-tracing frame gave; the camera pass then runs batch
	// frames 0, life, 2 life, ... — one per group spanned, group g from frame g x life.
	p.stale_retrace = in.cache_stale != 0 && p.first_retrace != 0;
	if(p.stale_retrace) { p.first_retrace = 0; p.n_retrace = p.n_groups; }
	p.n_pipes = p.m > 1 ? std::max(1, std::min(std::min(in.pipeline, kMaxPipes), p.m)) : 1;
	for(int k = 0; k < p.n_pipes; ++k) p.frames_of_pipe[k] = p.m / p.n_pipes + (k < p.m % p.n_pipes ? 1 : 0);
	// A single frame (no look-ahead, or one frame in flight) runs as a batch of one — camera launch, k_shade_first, k_path, k_resolve: 4 launches
	// instead of 1 + 2 x maxBounce — whenever a batch would take the one-launch pipeline (ADYPT_SINGLE_FUSED=0: the launch-per-bounce frame)
	p.kind = (p.m == 1 && in.single_fused && one_launch_ok(in, 1, 1)) ? PassPlan::Rolling : PassPlan::Batch;
	// (with the noise statistics on the lone launch-per-bounce frame is a batch of one too: it keeps its launches, its sample goes through k_resolve<true, *>)
	const bool lone = p.m == 1 && p.kind != PassPlan::Rolling;
	p.as_batch = !lone || in.noise_stats != 0;
	p.use_cache = p.as_batch || !p.n_retrace;
	p.fused_bounces = p.as_batch && !lone && one_launch_ok(in, p.m, p.n_pipes);
	// batches start every frame from a cached primary hit.  With the sun-visibility query on, k_shade_first only when k_path follows (it traces the
	// queries k_shade_first emits for the paths that escape at once); else the launch-per-bounce pipeline and its query queue
	p.fused_first = p.as_batch && in.first_fused && (!in.sun_visibility || p.fused_bounces);
	p.sun_query = in.sun_visibility && p.fused_bounces;
	p.sun_queue = in.sun_visibility && !p.fused_bounces;
	return p;
}

}  // namespace adypt
