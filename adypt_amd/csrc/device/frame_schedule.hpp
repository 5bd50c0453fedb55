// The frame scheduler behind adypt_trace_spp_async: frame_plan.hpp decides which pipeline a wavefront pass takes, the functions here enqueue it, step
// by step, in the order the launches reach the GPU.  A section of tracer.hip (included there only, after the launch helpers).  Results do not depend
// on the schedule: per-path work is independent of queue order and k_resolve applies the finished samples in frame order.
// A batch of several frames can be cut into sub-batches ("pipes"), each a chain on its OWN HIP stream over its own window of the ray queues: while one
// pipe's traversal launch drains (its last, longest rays) or its shade kernel streams the queues through HBM, the other pipe's traversal keeps the
// vector ALUs busy.
#pragma once
#include "context.hpp"
#include "../../../include/adypt_host.h"

namespace {

// what every launch of a pass is given besides its frames
struct PassArgs { SceneArgs sc; PixelArgs px; bool stats; };
PassArgs pass_args(const adypt_ctx *c)
{
	PassArgs a;
	fill_scene(c, &a.sc); fill_pixels(c, &a.px);
	a.stats = (c->instrumentation & 2) != 0;
	return a;
}

// The running-mean kernel over frames [first, first + count) of `f`'s parked samples, on the context's stream: with the noise statistics on the
// instance that keeps the luminance moments as well (noise.hpp); while blocks are frozen (they are only with the statistics on) the one with the slot
// map from the pass's pixels to the owned blocks' (active_blocks.hpp)
void launch_resolve(adypt_ctx *c, const FrameArgs &f, const PassArgs &a, int first, int count)
{
	const dim3 grid((c->pass_px + 255) / 256), block(256);
	NoiseMoments *const no_moments = nullptr;
	const int32_t *const no_slot = nullptr;
	if(c->ab.any_frozen()) hipLaunchKernelGGL((k_resolve<true, true>), grid, block, 0, c->stream, f, a.sc, a.px, c->d_noise_moments.get(), (const int32_t *)c->adaptive.slot, first, count);
	else if(c->noise_stats) hipLaunchKernelGGL((k_resolve<true, false>), grid, block, 0, c->stream, f, a.sc, a.px, c->d_noise_moments.get(), no_slot, first, count);
	else hipLaunchKernelGGL((k_resolve<false, false>), grid, block, 0, c->stream, f, a.sc, a.px, no_moments, no_slot, first, count);
}

// Running-mean step (pathtracer.glsl:224-226) of frames [first, first + count) of the batch last traced (its finished samples
// are parked in d_done), in frame order; afterwards image 1 holds the primary hits of the tmpLifetime group of the last frame
// applied — what frame-by-frame tracing leaves there (pathtracer.glsl:121-127).
int resolve_batch_frames(adypt_ctx *c, int first, int count)
{
	if(count <= 0) return ADYPT_OK;
	const PassArgs a = pass_args(c);
	FrameArgs f;
	fill_frame(c, &f);
	f.spp = c->batch_spp; f.n_frames = c->batch_frames;
	hipEvent_t stop = begin_timing(c, 1, c->stream);
	launch_resolve(c, f, a, first, count);
	end_timing(stop, c->stream);
	HIP_TRY(c, hipGetLastError());
	const int life = std::max(1, c->params.tmp_lifetime);
	const int group = (c->batch_spp + first + count - 1) / life - c->batch_spp / life;
	if(group > c->cache_group)
	{
		HIP_TRY(c, hipMemcpyAsync(c->d_cache, c->d_cache_next + (size_t)(group - 1) * (size_t)c->pass_px, (size_t)c->pass_px * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
		c->cache_group = group;
	}
	return ADYPT_OK;
}

// frames traced ahead belong to the camera / parameters / queues they were traced with: anything that changes those drops
// them (they are re-traced on demand — the sample sequence is a function of the frame index alone)
// The same for single frames whose k_path was started ahead in a rolling slot: waited for (their kernels read queues, counters and the camera's
// cache image) and forgotten.
void drop_rolling(adypt_ctx *c)
{
	if(c->roll_frame[0] < 0 && c->roll_frame[1] < 0) return;
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	for(int s = 0; s < 2; ++s) { (void)hipStreamSynchronize(c->pipes[1 + s].stream); c->roll_frame[s] = -1; }
}
inline void drop_lookahead(adypt_ctx *c) { c->ahead_count = 0; c->ahead_pos = 0; drop_rolling(c); }

// Sobol::Next (src/Util/Sobol.cpp:16-21) for frames [first, first + m): staged in a pinned slot, copied to `dst` on the context's stream
int upload_sobol(adypt_ctx *c, int first, int m, float *dst)
{
	const int max_bounce = c->params.max_bounce;
	const int slot = c->sobol_next;
	c->sobol_next = (slot + 1) % adypt_ctx::kSobolSlots;
	HIP_TRY(c, hipEventSynchronize(c->sobol_done[slot])); // the copy that last used this slot has left it
	std::vector<float> pts((size_t)m * 2 * max_bounce);
	int r = adypt_sobol_points(2 * max_bounce, first, m, pts.data());
	if(r != ADYPT_OK) return fail(c, r, adypt_host_last_error());
	float *padded = c->h_sobol[slot];
	memset(padded, 0, (size_t)m * 64 * sizeof(float));
	for(int k = 0; k < m; ++k) memcpy(&padded[(size_t)k * 64], &pts[(size_t)k * 2 * max_bounce], sizeof(float) * 2 * (size_t)max_bounce);
	HIP_TRY(c, hipMemcpyAsync(dst, padded, (size_t)m * 64 * sizeof(float), hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipEventRecord(c->sobol_done[slot], c->stream));
	return ADYPT_OK;
}

// Camera rays + bounce 0 of every frame of `f` from the cached primary hits, the surface fetched once per pixel and tmpLifetime group: k_shade_first on
// `stream`, with pipe `k`'s counters and audit bitmap; out = queue 1 = bounce 1's rays
void launch_shade_first(adypt_ctx *c, hipStream_t stream, int k, const QueueWindow &win, const FrameArgs &f, const PassArgs &a)
{
	FrameCounters *ctr = c->pipes[k].counters;
	hipEvent_t stop = begin_timing(c, 1, stream);
	QueueArgs q = queue_args(c, win, 0, ctr->count[0], ctr->count[1], f.n_frames);
	audit_before(c, q, stream, k);
	hipLaunchKernelGGL(k_shade_first, dim3((unsigned)(c->pass_px / kShadeThreads)), dim3(kShadeThreads), 0, stream, f, a.sc, q, a.px, a.stats ? 1 : 0);
	audit_after(c, q, stream, k);
	end_timing(stop, stream);
}

// the arguments of single frame `frame` in rolling slot `s`: a batch of one whose Sobol points, finished samples, queue window, counters and
// stream are the slot's
void roll_frame_args(const adypt_ctx *c, const PassPlan &p, int frame, int s, FrameArgs *f)
{
	fill_frame(c, f);
	f->spp = frame; f->n_frames = 1; f->frame_first = 0; f->frame_stride = 1; f->batched = 1;
	f->sun_query = p.sun_query; // (a rolling frame always takes the one-launch pipeline: the escaped paths' queries travel with it)
	f->sobol = c->d_sobol + (size_t)s * 64;
	f->done = c->q.done + (size_t)s * (size_t)std::max(c->n_local_px, 64);
}

// Enqueues single frame `frame` in rolling slot `s`: [camera rays of a re-tracing frame ->] counters -> k_shade_first on the CONTEXT's stream (it
// reads the primary-hit cache, which the next re-tracing frame rewrites on that stream), then k_path on the slot's own stream behind an event.
// Nothing here waits for the slot's previous frame: the caller has enqueued that frame's running-mean step — which waits for its k_path — on the
// context's stream before it calls this.
int roll_launch(adypt_ctx *c, const PassPlan &p, const PassArgs &a, int frame, int s)
{
	const Pipe &pipe = c->pipes[1 + s];
	const QueueWindow win = pipe_window(c, s, 2);
	FrameArgs f;
	roll_frame_args(c, p, frame, s, &f);
	int r = upload_sobol(c, frame, 1, c->d_sobol + (size_t)s * 64);
	if(r != ADYPT_OK) return r;
	if(frame % std::max(1, c->params.tmp_lifetime) == 0 || (p.stale_retrace && frame == c->spp))
	{
		// the frame re-traces its primary rays (pathtracer.glsl:113-127): one camera launch into the cache image, on the context's stream
		// (or stands in for its group's re-tracing frame behind a change of the block set: frame_plan.hpp stale_retrace)
		FrameArgs fc = f;
		fc.frame_stride = std::max(1, c->params.tmp_lifetime);
		r = launch_trace_camera(c, c->pipes[0], full_window(c), fc, a.px, 1, a.stats);
		if(r != ADYPT_OK) return r;
	}
	clear_counters(c, pipe.counters, 1, c->stream);
	launch_shade_first(c, c->stream, 1 + s, win, f, a);
	HIP_TRY(c, hipGetLastError());
	c->last_batch_fused = true;
	if(c->params.max_bounce > 1 || p.sun_query) // (with one bounce the queue still holds the sun-visibility queries of the paths that escaped at once)
	{
		HIP_TRY(c, hipEventRecord(c->roll_ready[s], c->stream));
		HIP_TRY(c, hipStreamWaitEvent(pipe.stream, c->roll_ready[s], 0));
		r = launch_path(c, pipe, win, 1, pipe.counters->count[1], pipe.counters->cursor[1], f, a.sc, a.px, 1, a.stats);
		if(r != ADYPT_OK) return r;
	}
	HIP_TRY(c, hipEventRecord(pipe.done, pipe.stream));
	c->roll_frame[s] = frame;
	return ADYPT_OK;
}

// frame c->spp as a rolling single frame (plan kind Rolling); `more` = the call wants the frame after it too
int trace_rolling_frame(adypt_ctx *c, const PassPlan &p, bool more)
{
	const PassArgs a = pass_args(c);
	const int frame = c->spp, s = frame & 1;
	// While frames come in order the slots hold nothing but `frame` (slot s: started ahead by the previous call) and `frame + 1` (slot s ^ 1); anything else
	// is waited for and forgotten first.
	if((c->roll_frame[s] >= 0 && c->roll_frame[s] != frame) || (c->roll_frame[s ^ 1] >= 0 && c->roll_frame[s ^ 1] != frame + 1)) drop_rolling(c);
	if(c->roll_frame[s] != frame)
	{
		const int r = roll_launch(c, p, a, frame, s);
		if(r != ADYPT_OK) { drop_rolling(c); return r; }
	}
	// The frame after it, when this call asks for it (or the caller switched look-ahead on and it belongs to the same tmpLifetime group, so that image 1
	// stays what frame-by-frame tracing leaves there): enqueued NOW, behind frame `frame`'s k_path — it fills the compute units as that launch's workgroups
	// end.  Its slot's previous frame (frame - 1) had its running-mean step enqueued by the previous call of this function.  Only while a frame is small
	// enough for the end of its launch to matter: at 4096 x 4096 (99 M rays, 14 ms per frame) the next frame's bounce 0 running beside the current k_path
	// costs the 3 % the launch's end is worth (6566 against 6777 Mrays/s, profiles/r5_ablations.txt 3).
	const int life = std::max(1, c->params.tmp_lifetime);
	const bool ahead = c->single_overlap && c->n_local_px <= kRollMaxPixels && (more || (c->lookahead && (frame + 1) % life != 0));
	if(ahead && c->roll_frame[s ^ 1] != frame + 1)
	{
		const int r = roll_launch(c, p, a, frame + 1, s ^ 1);
		if(r != ADYPT_OK) { drop_rolling(c); return r; }
	}
	// running mean of frame `frame` (pathtracer.glsl:224-226) once its k_path has ended
	HIP_TRY(c, hipStreamWaitEvent(c->stream, c->pipes[1 + s].done, 0));
	FrameArgs f;
	roll_frame_args(c, p, frame, s, &f);
	hipEvent_t stop = begin_timing(c, 1, c->stream);
	launch_resolve(c, f, a, 0, 1);
	end_timing(stop, c->stream);
	HIP_TRY(c, hipGetLastError());
	c->roll_frame[s] = -1;
	c->batch_spp = frame; c->batch_frames = 1; c->cache_group = 0; c->ahead_pos = 1; c->ahead_count = 0;
	c->spp += 1;
	return ADYPT_OK;
}


// ---- a batch (plan kind Batch): re-trace pass -> fork -> bounce 0 per pipe -> k_path | bounce by bounce -> join -> k_resolve ----

// One sub-batch of a batch: its window of the queues, its frames, the grid of its launch-per-bounce kernels (kNumSegments x chunks per segment)
struct SubBatch { QueueWindow win; FrameArgs f; int grid; };

// The main pass, cut into n_pipes sub-batches of consecutive frames; sub-batch k runs on pipe k's stream in window k of the queues
void cut_sub_batches(adypt_ctx *c, const PassPlan &p, SubBatch *sub)
{
	FrameArgs f;
	fill_frame(c, &f);
	f.batched = p.as_batch ? 1 : 0; f.sun_query = p.sun_query ? 1 : 0;
	for(int k = 0, frame0 = 0; k < p.n_pipes; ++k)
	{
		sub[k].win = pipe_window(c, k, p.n_pipes);
		sub[k].f = f;
		sub[k].f.n_frames = p.frames_of_pipe[k]; sub[k].f.frame_first = frame0;
		sub[k].grid = (int)(kNumSegments * (pass_seg_paths(c, sub[k].win, p.frames_of_pipe[k]) / kShadeThreads));
		frame0 += p.frames_of_pipe[k];
	}
}

// primary-only pass of the re-tracing frames: camera rays -> traversal -> cache image of each frame's group
// (on the context's stream, in the whole queue: every sub-batch starts from these cache images)
int launch_retrace_pass(adypt_ctx *c, const PassPlan &p, const PassArgs &a)
{
	FrameArgs f;
	fill_frame(c, &f);
	f.batched = 1; f.n_frames = p.n_retrace; f.frame_first = p.first_retrace; f.frame_stride = std::max(1, c->params.tmp_lifetime);
	return launch_trace_camera(c, c->pipes[0], full_window(c), f, a.px, 1, a.stats);
}

// bounce 0 of sub-batch k without k_shade_first: new paths into queue 0 (the lone frame that re-traces: as camera rays for bounce 0's traversal)
void launch_gen_primary(adypt_ctx *c, const PassPlan &p, const PassArgs &a, const SubBatch &sb, int k)
{
	const Pipe &pipe = c->pipes[k];
	hipEvent_t stop = begin_timing(c, 1, pipe.stream);
	QueueArgs q = queue_args(c, sb.win, 1, pipe.counters->count[0], pipe.counters->count[0], sb.f.n_frames); // out = queue 0
	audit_before(c, q, pipe.stream, k);
	hipLaunchKernelGGL(k_gen_primary, dim3(sb.grid), dim3(kShadeThreads), 0, pipe.stream, sb.f, a.sc, q, a.px, p.use_cache ? 1 : 0, 1);
	audit_after(c, q, pipe.stream, k);
	end_timing(stop, pipe.stream);
}

// the escaped paths of bounce b (plan: sun_queue): any-hit query towards the sun, then sun term + accumulate (pathtracer.glsl:130-135)
int launch_sun_queries(adypt_ctx *c, const PassArgs &a, const SubBatch &sb, int k, int b, const QueueArgs &q, const ShadowArgs &sh)
{
	const Pipe &pipe = c->pipes[k];
	int r = launch_trace(c, pipe, sb.win, 0, pipe.counters->sh_count[b], pipe.counters->sh_cursor[b], c->params.stack_size, a.stats, nullptr, true, true);
	if(r != ADYPT_OK) return r;
	hipEvent_t stop = begin_timing(c, 1, pipe.stream);
	hipLaunchKernelGGL(k_shadow_resolve, dim3(sb.grid), dim3(kShadeThreads), 0, pipe.stream, sb.f, q, a.px, sh);
	end_timing(stop, pipe.stream);
	return ADYPT_OK;
}

// bounce b of sub-batch k in the launch-per-bounce pipeline: k_trace -> k_shade [-> the sun-visibility queries]
int launch_bounce(adypt_ctx *c, const PassPlan &p, const PassArgs &a, const SubBatch &sb, int k, int b)
{
	const Pipe &pipe = c->pipes[k];
	FrameCounters *ctr = pipe.counters;
	const int in = b & 1;
	if(!(b == 0 && p.use_cache))
	{
		int r = launch_trace(c, pipe, sb.win, in, ctr->count[b], ctr->cursor[b], c->params.stack_size, a.stats, nullptr, false, false, true, b == 0); // (b == 0: camera rays from the queue, tile by tile)
		if(r != ADYPT_OK) return r;
	}
	QueueArgs q = queue_args(c, sb.win, in, ctr->count[b], ctr->count[b + 1], sb.f.n_frames);
	ShadowArgs sh;
	sh.o = c->q.sh_o + sb.win.offset; sh.d = c->q.sh_d + sb.win.offset; sh.col = c->q.sh_col + sb.win.offset; sh.hit = c->q.sh_hit + sb.win.offset;
	sh.count = ctr->sh_count[b];
	memcpy(sh.dir, c->sun_dir, sizeof(sh.dir));
	sh.enabled = p.sun_queue ? 1 : 0;
	hipEvent_t stop = begin_timing(c, 1, pipe.stream);
	audit_before(c, q, pipe.stream, k);
	hipLaunchKernelGGL(k_shade, dim3(sb.grid), dim3(kShadeThreads), 0, pipe.stream, sb.f, a.sc, q, a.px, sh, b, (b == 0 && !p.use_cache) ? 1 : 0, a.stats ? 1 : 0);
	audit_after(c, q, pipe.stream, k);
	end_timing(stop, pipe.stream);
	return p.sun_queue ? launch_sun_queries(c, a, sb, k, b, q, sh) : ADYPT_OK;
}

// Everything between the fork and the join of the pipes' streams.  What was enqueued before (Sobol upload, re-trace pass, the previous batch's
// k_resolve, the clearing of the counters) is ordered before every chain by the fork event, every chain before k_resolve by the join.
int enqueue_chains(adypt_ctx *c, const PassPlan &p, const PassArgs &a, const SubBatch *sub)
{
	if(p.n_pipes > 1)
	{
		HIP_TRY(c, hipEventRecord(c->fork_ev, c->stream));
		for(int k = 1; k < p.n_pipes; ++k) HIP_TRY(c, hipStreamWaitEvent(c->pipes[k].stream, c->fork_ev, 0));
	}
	for(int k = 0; k < p.n_pipes; ++k)
	{
		if(p.fused_first) launch_shade_first(c, c->pipes[k].stream, k, sub[k].win, sub[k].f, a);
		else launch_gen_primary(c, p, a, sub[k], k);
	}
	c->last_batch_fused = p.fused_bounces;
	if(p.fused_bounces)
	{
		// every bounce after the first in ONE launch (k_path): the reference's for(b < uMaxBounce) inside a single dispatch
		const Pipe &pipe = c->pipes[0];
		if(c->params.max_bounce > 1 || p.sun_query)
		{
			int r = launch_path(c, pipe, sub[0].win, 1, pipe.counters->count[1], pipe.counters->cursor[1], sub[0].f, a.sc, a.px, 1, a.stats);
			if(r != ADYPT_OK) return r;
		}
	}
	else for(int b = p.fused_first ? 1 : 0; b < c->params.max_bounce; ++b)
		for(int k = 0; k < p.n_pipes; ++k) // bounce by bounce over the pipes: their launches reach the GPU interleaved
		{
			int r = launch_bounce(c, p, a, sub[k], k, b);
			if(r != ADYPT_OK) return r;
		}
	for(int k = 1; k < p.n_pipes; ++k)
	{
		HIP_TRY(c, hipEventRecord(c->pipes[k].done, c->pipes[k].stream));
		HIP_TRY(c, hipStreamWaitEvent(c->stream, c->pipes[k].done, 0));
	}
	HIP_TRY(c, hipGetLastError());
	return ADYPT_OK;
}

// frames [c->spp, c->spp + p.m) as one wavefront; the first p.hand_out of them go into the image
int enqueue_batch(adypt_ctx *c, const PassPlan &p)
{
	drop_rolling(c); // (a batch works in the whole queues)
	int r;
	if(p.as_batch && p.n_groups > 1 && (r = ensure_cache_slices(c, p.n_groups - 1)) != ADYPT_OK) return r;
	const PassArgs a = pass_args(c);
	if((r = upload_sobol(c, c->spp, p.m, c->d_sobol)) != ADYPT_OK) return r;
	if(p.as_batch && p.n_retrace && (r = launch_retrace_pass(c, p, a)) != ADYPT_OK) return r;
	if(p.sun_queue && (r = ensure_shadow_queue(c)) != ADYPT_OK) return r;
	SubBatch sub[kMaxPipes];
	cut_sub_batches(c, p, sub);
	// the counters of all pipes are contiguous: one clearing launch, on the context's stream, before the chains fork
	clear_counters(c, c->d_counters, p.n_pipes, c->stream);
	r = enqueue_chains(c, p, a, sub);
	if(r != ADYPT_OK)
	{
		// a launch or HIP call that fails between the fork and the join must not leave the other chains running unjoined: what follows on the
		// context's stream (or the caller's next call) only synchronises c->stream, and those chains would still be writing queues, done[] and counters
		for(int k = 1; k < kMaxPipes; ++k) (void)hipStreamSynchronize(c->pipes[k].stream);
		return r;
	}
	if(p.as_batch)
	{
		c->batch_spp = c->spp; c->batch_frames = p.m; c->cache_group = 0;
		if((r = resolve_batch_frames(c, 0, p.hand_out)) != ADYPT_OK) return r;
		c->ahead_pos = p.hand_out; c->ahead_count = p.m - p.hand_out;
	}
	c->spp += p.hand_out;
	return ADYPT_OK;
}

// ---- the steps of adypt_trace_spp_async ----

// k frames already traced ahead by an earlier call: only their running-mean step is left (frame order is kept)
int hand_out_parked(adypt_ctx *c, int k)
{
	int r = resolve_batch_frames(c, c->ahead_pos, k);
	if(r != ADYPT_OK) return r;
	c->ahead_pos += k; c->ahead_count -= k; c->spp += k;
	return ADYPT_OK;
}

// first path-traced frame (OglPathTracer.cpp:39-46): apply config, clear the result image, restart Sobol
int start_path_tracing(adypt_ctx *c)
{
	int r = apply_params(c);
	if(r != ADYPT_OK) return r;
	HIP_TRY(c, hipMemsetAsync(c->d_accum, 0, (size_t)std::max(c->n_local_px, 64) * sizeof(float4), c->stream));
	c->spp = 0;
	c->pt_started = true;
	c->view_type = 3; // kPTRadiance (OglPathTracer.cpp:38)
	return ADYPT_OK;
}

PlanInput plan_input(const adypt_ctx *c, int remaining)
{
	return PlanInput{c->spp, remaining, c->lookahead, c->frames_in_flight, c->params.tmp_lifetime, c->params.max_bounce, c->pipeline,
	                 c->single_fused, c->first_fused, c->fused_bounces, c->sun_visibility, c->pass_px, c->noise_stats, c->cache_stale ? 1 : 0};
}

}  // namespace
