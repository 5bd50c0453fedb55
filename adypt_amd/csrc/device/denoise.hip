// The denoiser (include/adypt_hip.h adypt_denoise ...; the definition: denoise.hpp).  A translation unit of its own: nothing here is part of the
// tracer's code object.  What runs, all on the context's stream behind the frames:
//     guide capture  three launches of the viewer instance of k_trace_camera over the owned blocks (tracer.hip ctx_capture_guides), into scratch
//                    owned here: albedo, normal, position, primary hit — block-major like every local image
//     k_chain_start, k_chain_step  adypt_denoise_specular only (the definition: guide_chain.hpp), behind the capture: pixels whose primary hit is a perfect
//                    mirror or glass are followed for up to K bounces — k_chain_start classifies every local pixel and writes a ray for those that go on,
//                    then K rounds of the context's own k_trace over its ray queues (ctx_ray_queues, ctx_trace_queue) and k_chain_step, which ends a
//                    pixel (albedo, normal, position into the guide scratch, the class into the .w of its primary hit) or writes the next ray
//     k_denoise_prepare  block-major accum / moments / block sample counts / guides  ->  row-major float4 images X0 = (D0.rgb, V0), X1 = (N.xyz, hit),
//                    X2 = (P.xyz, n), XA = (A.rgb, .); k_denoise_prepare_class (followed guides): X1.w is the pixel's class instead of the hit flag
//     k_temporal_merge  adypt_denoise_temporal only (the definition: temporal.hpp): the history the last committing call left — its merged pre-filter
//                    (D, V), its guides, its effective sample counts, its camera — reprojected through P and merged into (D0, V0); the levels then
//                    read the merged image.  A commit swaps the call's images with the history's: nothing is copied
//     k_chain_start<true>, k_chain_step<true>, k_denoise_prepare_virtual, k_temporal_merge_virtual  adypt_denoise_temporal_specular only: the chain
//                    also unfolds the camera ray to its full length and leaves the VIRTUAL POINT of every pixel that ends on a surface (block-major,
//                    kVirtual); prepare brings it to the picture's coordinates, XV = (Pv.xyz, len), and the merge reprojects a followed pixel through it,
//                    holding every tap against the followed guides and the pixel's class (temporal.hpp temporal_merge_virtual).  The order of such a
//                    call: guide capture -> chain -> prepare -> merge -> levels, on the context's stream without a host sync until the end
//     k_motion_gather  adypt_denoise_temporal_motion only, before the merge and inside its stage of the timer: per pixel the hit triangle's words 0..17
//                    as the last committing motion call left them (the snapshot) against the record as it is now -> where the hit point and its normal
//                    WERE then (temporal_previous_point), row-major XP = (P_prev.xyz, moved), XN = (N_prev.xyz, valid); k_temporal_merge<true> merges
//                    through them.  k_motion_snapshot, on such a call's commit: the first 80 bytes of every record into the snapshot
//     k_rectify_window<R>  a rectified call only (the definition: rectify.hpp), before the merge and inside its stage of the timer: per pixel the mean of the
//                    (2 R + 1)^2 window of the call's own images on the pixel's surface and the squared limit a history value may lie from it, row-major
//                    R0 = (mu.rgb, k), R1 = (g.rgb, 0); k_temporal_merge<., true> clamps the history to them and writes the share of its length it kept
//     k_moments_variance  a moments call only (the definition: moments.hpp), behind the merge and inside its stage of the timer: such a call's prepare
//                    (k_denoise_prepare_moments) and merge (k_temporal_merge_moments) carry the raw second moment S where the variance stands;
//                    this kernel makes the variance of every pixel from the merged (D, S) and n_out — a 7 x 7 window of the merged image where the
//                    history is short — and writes (D, V) into X0, which the first level then reads.  The merged (D, S) is what a commit leaves
//     k_atrous<LAST>  one level per launch, X0 ping-pongs; the last level multiplies the albedo back and writes the W x H x 3 result
// Several devices: every context captures the guides of its own blocks, the host puts the devices' local images back to back in rank order, their
// block lists likewise (every block has one owner, and k_denoise_prepare takes any block list and writes at the picture's coordinates), uploads them
// to the first device and runs the same kernels there (the merge too: the history lives on the first device) — no collective; the result is the
// one-device result bit for bit because the inputs are.
// The host side, in the order of the file:
//     BlockImages   the block-major images of a set of blocks on one device, named once (BlockImage) and handled in loops: the context's own set
//                   and, on the first device of several, the merged set of all devices.  LocalImages is the view of a set the kernels are launched with
//     History       what the last committing call left, its kind (HistoryKind), its camera and its snapshot.  Its methods are the lifetime rule and
//                   its only writers
//     the stages    one struct per stage that only some calls have — MergeStage, MotionStage, WindowStage, MomentsStage, VirtualStage, ChainStage —
//                   each with its buffers, its read-out flag, its timer, counters and last parameters, and the same members: ensure, enqueue,
//                   finished, fill
//     Denoiser      everything kept per context: the picture's images, the history, the stages.  While timer.completed(), `last` says what the last
//                   finished run was, and rgb is its result
//     run_filter    the steps of a call (denoise_call.hpp: DenoiseCall, made once from the ABI structs by make_call) over a set of images, in order:
//                   prepare, [gather], [window], merge, [variance], levels, [snapshot], sync, finished; denoise_context and multi_denoise are the fronts
#include "ctx_unit.hpp"
#include "tile_layout.hpp"
#include "denoise_call.hpp"
#include "denoise_internal.hpp"
#include "../../../include/adypt_hip.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace adypt;

#include "denoise_kernels.hpp" // the kernels, in this unit's anonymous namespace, and the shape each is launched with (the probe library compiles them too)

namespace {

// The block-major images of a set of blocks on one device, in the order the several-device path uploads them: the first kPixelImages hold one element
// per local pixel, the last two one per block.  A further image is one more name here, its element type where that is not float4, its size in the table
// and, if it is per pixel, its place in kFetchOrder.
// kVirtual — the virtual points of a call by the virtual point — is allocated, fetched and uploaded by such a call only (optional_images).
enum BlockImage { kAccum, kAlbedo, kNormal, kPosition, kHits, kMoments, kVirtual, kBlocks, kBlockSpp, kBlockImages, kPixelImages = kBlocks };
template <BlockImage K> struct ImageElement { using type = float4; };
template <> struct ImageElement<kMoments> { using type = float2; };
template <> struct ImageElement<kBlocks> { using type = int32_t; };
template <> struct ImageElement<kBlockSpp> { using type = int32_t; };
template <BlockImage K> constexpr size_t block_bytes() { return sizeof(typename ImageElement<K>::type) * (K < kPixelImages ? kBlockPixels : 1); }
constexpr size_t kBlockImageBytes[] = {block_bytes<kAccum>(), block_bytes<kAlbedo>(), block_bytes<kNormal>(), block_bytes<kPosition>(),
                                       block_bytes<kHits>(), block_bytes<kMoments>(), block_bytes<kVirtual>(), block_bytes<kBlocks>(), block_bytes<kBlockSpp>()}; // of one block
static_assert(sizeof(kBlockImageBytes) / sizeof(size_t) == kBlockImages, "every block-major image has its size");
// the order in which the several-device path fetches a device's per-pixel images (the uploads go in the enum's order)
constexpr BlockImage kFetchOrder[] = {kMoments, kAccum, kAlbedo, kNormal, kPosition, kHits, kVirtual};
static_assert(sizeof(kFetchOrder) / sizeof(BlockImage) == kPixelImages, "every per-pixel image is fetched");
constexpr unsigned kContextImages = 1u << kAccum | 1u << kMoments | 1u << kBlocks; // the images a context keeps itself (DenoiseInputs)
// the images a call goes without — neither allocated nor moved between devices, and null in its LocalImages
constexpr unsigned kWithoutVirtual = 1u << kVirtual;
inline unsigned optional_images(const DenoiseCall &call) { return call.virtual_point() ? 0u : kWithoutVirtual; }

// where the images of a set of n_blocks blocks lie: what the kernels are launched with
struct LocalImages {
	const void *image[kBlockImages];
	int n_blocks;
	template <BlockImage K> const typename ImageElement<K>::type *as() const { return (const typename ImageElement<K>::type *)image[K]; }
};

// The buffers of a set, grow-only.  The context's own set borrows the kContextImages from the context (64 B per local pixel + 4 B per owned block remain:
// the guides and the sample counts); the merged set of all devices, on the first device, owns every image (88 B per pixel + 8 B per block).
struct BlockImages {
	Buffer<uint8_t> image[kBlockImages];
	template <BlockImage K> typename ImageElement<K>::type *as() const { return (typename ImageElement<K>::type *)image[K].get(); }
	// room for v->n_blocks blocks in every image but the `borrowed` ones (a mask of 1 << BlockImage), which stay what the caller made them, null included
	int fill(adypt_ctx *c, LocalImages *v, unsigned borrowed)
	{
		for(int k = 0; k < kBlockImages; ++k)
			if(!(borrowed >> k & 1))
			{
				CTX_TRY(c, at_least(image[k], (size_t)v->n_blocks * kBlockImageBytes[k]));
				v->image[k] = image[k].get();
			}
		return ADYPT_OK;
	}
};

// The history of the temporal merge: what the last committing call left — its merged image, its X1, X2 with n_out in .w, XA (64 B per image pixel,
// allocated at the first temporal call) and its camera — and the snapshot, which belongs to it: the first 80 bytes of every triangle record as a
// committing motion call found them, allocated at the first such call.  The methods are the lifetime rule, and nothing else writes a member: the
// snapshot is written only by a committing motion call; dropped by reset, by a committing call without motion (the history's geometry is then unknown)
// and by adypt_set_triangles (the indices mean other triangles).
struct History {
	Buffer<float4> h0, h1, h2, ha;
	TemporalCamera camera;
	bool present = false;
	HistoryKind kind;                // of the call that wrote it: a call finds only a history of its own kind
	Buffer<float4> snapshot;
	int64_t snapshot_tris = 0;       // the triangles the snapshot holds; 0: the history has none (a context's scene never has 0: adypt_create, adypt_set_triangles)
	StageTimer<2> snapshot_timer;    // the copy kernel of the last commit with a snapshot

	int ensure(adypt_ctx *c, size_t n_px)
	{
		CTX_TRY(c, at_least(h0, n_px)); CTX_TRY(c, at_least(h1, n_px)); CTX_TRY(c, at_least(h2, n_px)); CTX_TRY(c, at_least(ha, n_px));
		return ADYPT_OK;
	}
	// how many triangles of the snapshot the gather may trust for a scene of n_tris triangles (a snapshot of another count is none: adypt_set_triangles
	// drops it, so this only guards)
	int64_t known_tris(int64_t n_tris) const { return present && snapshot_tris == n_tris ? snapshot_tris : 0; }
	int found_by(const DenoiseCall &call) const { return present && kind == call.kind() ? 1 : 0; } // (the `have` of the merge kernels)
	// The snapshot of a committing motion call: the records as they are now, enqueued on `stream` behind the call's gather, which reads the old one.  The
	// history has none from here until the caller has waited for the stream and commits with *n_tris: a failure in between leaves every pixel unmoved.
	int enqueue_snapshot(adypt_ctx *c, hipStream_t stream, int64_t *n_tris)
	{
		const CtxScene sc = ctx_scene(c);
		snapshot_tris = 0;
		CTX_TRY(c, at_least(snapshot, (size_t)(sc.n_tris * kSnapshotVecs)));
		CTX_TRY(c, snapshot_timer.mark(0, stream));
		const LaunchShape copy = snapshot_launch(sc.n_tris);
		hipLaunchKernelGGL(k_motion_snapshot, copy.grid, copy.block, 0, stream, (const float4 *)sc.triangles, sc.tri_float4, sc.n_tris, snapshot.get());
		CTX_TRY(c, hipGetLastError());
		CTX_TRY(c, snapshot_timer.mark(1, stream));
		*n_tris = sc.n_tris;
		return ADYPT_OK;
	}
	// A finished call's merged image, guides (X2.w = n_out) and camera become the history: swapped in, nothing is copied, and what the history held is
	// overwritten by the call's next prepare.  snapshot_of: what enqueue_snapshot gave; 0: the call made none, and the history has none from here.
	void commit(Buffer<float4> &merged, Buffer<float4> &x1, Buffer<float4> &x2, Buffer<float4> &xa, const CtxCamera &cam, int64_t snapshot_of, const HistoryKind &of_call)
	{
		kind = of_call;
		std::swap(merged, h0); std::swap(x1, h1); std::swap(x2, h2); std::swap(xa, ha);
		camera = temporal_camera(cam.origin, cam.inv_proj, cam.inv_view);
		snapshot_tris = snapshot_of;
		present = true;
	}
	void reset() { present = false; snapshot_tris = 0; } // (the memory stays)
	// the snapshot's indices mean other triangles now; its memory is given back (adypt_get_denoise_motion reports it).  The history itself stays
	void triangles_replaced() { snapshot_tris = 0; snapshot.release(); }
};

// the filter's row-major images of the whole picture as the kernels of one call are launched with them (x0: what prepare writes and level 0 leaves)
struct Picture {
	float4 *x0, *x1, *x2, *xa;
	int width, height;
	int blocks_x() const { return (width + kBlockDim - 1) / kBlockDim; }
};

// ---- the stages that only some calls have ----
// Each keeps what its calls leave for the read-outs, and the same members.  ensure(c, n): room for a picture of n pixels, and the read-out invalid
// from here — it is called before anything that can overwrite the stage's images is enqueued.  enqueue: the stage's kernels, on the call's stream.
// finished(call): behind the wait for the stream; a call that has the stage makes its read-out valid and leaves its parameters and counts, a call
// of another kind changes nothing — so a read-out answers from the first call of its kind that ran to its end, and a call that failed leaves it
// refused until the next one has.  fill: the stage's adypt_denoise_* struct, zeroed by the caller; device_bytes whether or not a call has run.
// Nothing outside a stage writes its `valid`.

// following moved geometry (adypt_denoise_temporal_motion, the rectified and the moments call with follow_motion): XP, XN, 32 B per image pixel,
// allocated at the first such call.  (The snapshot is the history's: it lives and dies with what was committed.)
struct MotionStage {
	Buffer<float4> xp, xn;
	bool valid = false;
	int ensure(adypt_ctx *c, size_t n) { valid = false; CTX_TRY(c, at_least(xp, n)); CTX_TRY(c, at_least(xn, n)); return ADYPT_OK; }
	// k_motion_gather: where every pixel's hit point and normal were when the history was committed
	int enqueue(adypt_ctx *c, hipStream_t stream, const LocalImages &in, const Picture &px, const History &h)
	{
		const CtxScene sc = ctx_scene(c);
		const int n_px = in.n_blocks * kBlockPixels;
		const LaunchShape gather = gather_launch(n_px);
		hipLaunchKernelGGL(k_motion_gather, gather.grid, gather.block, 0, stream, in.as<kHits>(), in.as<kNormal>(), in.as<kPosition>(), in.as<kBlocks>(), n_px, px.blocks_x(), px.width, px.height,
		                   (const float4 *)h.snapshot, h.known_tris(sc.n_tris), (const float4 *)sc.triangles, sc.tri_float4, xp.get(), xn.get());
		CTX_TRY(c, hipGetLastError());
		return ADYPT_OK;
	}
	void finished(const DenoiseCall &call) { if(call.motion) valid = true; }
	void fill(const History &h, adypt_denoise_motion *out) const
	{
		out->have_snapshot = h.snapshot_tris > 0 ? 1 : 0;
		out->n_tris = h.snapshot_tris;
		out->device_bytes = (int64_t)(h.snapshot.bytes() + xp.bytes() + xn.bytes());
		if(out->have_snapshot) (void)h.snapshot_timer.read(&out->snapshot_ms, 1, 1, false);
	}
};

// rectifying stale history (rectify.hpp): R0, R1 and the kept read-out, 36 B per image pixel, allocated at the first rectified call; the parameters and
// the window kernel's time of the last one
struct WindowStage {
	Buffer<float4> r0, r1;
	Buffer<float> kept;
	bool valid = false;
	int radius = 0; float gamma = 0.0f;
	StageTimer<2> timer;
	int ensure(adypt_ctx *c, size_t n) { valid = false; CTX_TRY(c, at_least(r0, n)); CTX_TRY(c, at_least(r1, n)); CTX_TRY(c, at_least(kept, n)); return ADYPT_OK; }
	// k_rectify_window<call.radius>: the window statistics of the call's own images, which the merge then clamps the history to
	int enqueue(adypt_ctx *c, hipStream_t stream, const Picture &px, const RectifyOrigin &origin, const DenoiseCall &call)
	{
		const LaunchShape shape = window_launch(px.width, px.height);
		CTX_TRY(c, timer.mark(0, stream));
		hipLaunchKernelGGL(window_instance(call.radius), shape.grid, shape.block, 0, stream, (const float4 *)px.x0, (const float4 *)px.x1, (const float4 *)px.x2, (const float4 *)px.xa, r0.get(), r1.get(),
		                   px.width, px.height, origin);
		CTX_TRY(c, hipGetLastError());
		CTX_TRY(c, timer.mark(1, stream));
		return ADYPT_OK;
	}
	void finished(const DenoiseCall &call) { if(call.rectify) { valid = true; radius = call.radius; gamma = call.gamma; } }
	void fill(adypt_denoise_rectify *out) const
	{
		out->device_bytes = (int64_t)(r0.bytes() + r1.bytes() + kept.bytes());
		if(!valid) return;
		out->have = 1;
		out->radius = radius; out->gamma = gamma;
		(void)timer.read(&out->window_ms, 1, 1, false);
	}
};

// variance from temporal moments (moments.hpp): the variance read-out, 4 B per image pixel, and the counters of the pixels that took the window
// estimate (512 B), allocated at the first moments call; the count and the variance kernel's time of the last one
struct MomentsStage {
	Buffer<float> variance;
	Buffer<unsigned long long> count;
	bool valid = false;
	int64_t pixels_spatial = 0;
	unsigned long long readback[kMomentsCountSlots] = {}; // where the running call's counters are copied to (a member: the copy is enqueued, and outlives a call that fails behind it)
	StageTimer<2> timer;
	int ensure(adypt_ctx *c, size_t n) { valid = false; CTX_TRY(c, at_least(variance, n)); CTX_TRY(c, at_least(count, kMomentsCountSlots)); return ADYPT_OK; }
	// k_moments_variance: (D, V) of the merged (D, S) into X0, which the merge has read and the first level reads; the merged image itself stays for the commit
	int enqueue(adypt_ctx *c, hipStream_t stream, const Picture &px, const float4 *merged, const RectifyOrigin &origin)
	{
		const LaunchShape shape = variance_launch(px.width, px.height);
		CTX_TRY(c, hipMemsetAsync(count.get(), 0, sizeof(readback), stream));
		CTX_TRY(c, timer.mark(0, stream));
		hipLaunchKernelGGL(k_moments_variance, shape.grid, shape.block, 0, stream, merged, (const float4 *)px.x1, (const float4 *)px.x2, (const float4 *)px.xa, px.x0, variance.get(), count.get(), px.width,
		                   px.height, origin);
		CTX_TRY(c, hipGetLastError());
		CTX_TRY(c, timer.mark(1, stream));
		CTX_TRY(c, hipMemcpyAsync(readback, count.get(), sizeof(readback), hipMemcpyDeviceToHost, stream));
		return ADYPT_OK;
	}
	void finished(const DenoiseCall &call)
	{
		if(!call.moments) return;
		valid = true;
		pixels_spatial = 0;
		for(const unsigned long long n_slot : readback) pixels_spatial += (int64_t)n_slot;
	}
	void fill(adypt_denoise_moments *out) const
	{
		out->device_bytes = (int64_t)(variance.bytes() + count.bytes());
		if(!valid) return;
		out->have = 1;
		out->pixels_spatial = pixels_spatial;
		(void)timer.read(&out->variance_ms, 1, 1, false);
	}
};

// the temporal merge by the virtual point: XV, 16 B per image pixel, and the counters (1 KiB), allocated at the first such call (the block-major
// virtual points, 16 B per local pixel, are the block-image sets' kVirtual); the bounces and the counts of the last one
struct VirtualStage {
	Buffer<float4> xv;
	Buffer<unsigned long long> count;
	bool valid = false;
	int bounces = 0;
	int64_t followed = 0, with_history = 0;
	unsigned long long readback[2 * kVirtualCountSlots] = {}; // (a member, as MomentsStage's)
	int ensure(adypt_ctx *c, size_t n) { valid = false; CTX_TRY(c, at_least(xv, n)); CTX_TRY(c, at_least(count, 2 * kVirtualCountSlots)); return ADYPT_OK; }
	// k_temporal_merge_virtual: such a call's merge, into `merged` and `length`
	int enqueue(adypt_ctx *c, hipStream_t stream, const Picture &px, const History &h, const DenoiseCall &call, float4 *merged, float *length)
	{
		const LaunchShape shape = merge_launch(px.width, px.height);
		CTX_TRY(c, hipMemsetAsync(count.get(), 0, sizeof(readback), stream));
		hipLaunchKernelGGL(k_temporal_merge_virtual, shape.grid, shape.block, 0, stream, (const float4 *)px.x0, (const float4 *)px.x1, px.x2, (const float4 *)px.xa, (const float4 *)xv, (const float4 *)h.h0,
		                   (const float4 *)h.h1, (const float4 *)h.h2, (const float4 *)h.ha, merged, length, px.width, px.height, h.found_by(call), h.camera, call.history_cap, count.get());
		CTX_TRY(c, hipMemcpyAsync(readback, count.get(), sizeof(readback), hipMemcpyDeviceToHost, stream));
		return ADYPT_OK;
	}
	void finished(const DenoiseCall &call)
	{
		if(!call.virtual_point()) return;
		valid = true; bounces = call.bounces;
		followed = with_history = 0;
		for(int k = 0; k < kVirtualCountSlots; ++k) { followed += (int64_t)readback[2 * k]; with_history += (int64_t)readback[2 * k + 1]; }
	}
	// block_major_bytes: of the virtual points the context's block-image sets hold
	void fill(size_t block_major_bytes, adypt_denoise_virtual *out) const
	{
		out->device_bytes = (int64_t)(block_major_bytes + xv.bytes() + count.bytes());
		if(!valid) return;
		out->have = 1; out->bounces = bounces;
		out->pixels_followed = followed; out->pixels_with_history = with_history;
	}
};

// every call with history: the merged image of the call and the length read-out, 20 B per image pixel, allocated at the first such call
struct MergeStage {
	Buffer<float4> xm;
	Buffer<float> length;
	bool valid = false;
	int ensure(adypt_ctx *c, size_t n) { valid = false; CTX_TRY(c, at_least(xm, n)); CTX_TRY(c, at_least(length, n)); return ADYPT_OK; }
	// the merge of the call's form: by the virtual point, of a moments call, or k_temporal_merge<call.motion, call.rectify>.  (An instance never looks at
	// the images of a stage its call has not: they may be null.)
	int enqueue(adypt_ctx *c, hipStream_t stream, const Picture &px, const History &h, const DenoiseCall &call, const MotionStage &motion, const WindowStage &window, VirtualStage &virt)
	{
		if(call.virtual_point()) CTX_STEP(virt.enqueue(c, stream, px, h, call, xm.get(), length.get()));
		else
		{
			const LaunchShape shape = merge_launch(px.width, px.height);
			if(call.moments)
				hipLaunchKernelGGL(merge_moments_instance(call.motion), shape.grid, shape.block, 0, stream, (const float4 *)px.x0, (const float4 *)px.x1, px.x2, (const float4 *)px.xa, (const float4 *)h.h0,
				                   (const float4 *)h.h1, (const float4 *)h.h2, (const float4 *)h.ha, xm.get(), length.get(), px.width, px.height, h.found_by(call), h.camera, call.history_cap,
				                   (const float4 *)motion.xp, (const float4 *)motion.xn);
			else
				hipLaunchKernelGGL(merge_instance(call.motion, call.rectify), shape.grid, shape.block, 0, stream, (const float4 *)px.x0, (const float4 *)px.x1, px.x2, (const float4 *)px.xa, (const float4 *)h.h0,
				                   (const float4 *)h.h1, (const float4 *)h.h2, (const float4 *)h.ha, xm.get(), length.get(), px.width, px.height, h.found_by(call), h.camera, call.history_cap,
				                   (const float4 *)motion.xp, (const float4 *)motion.xn, (const float4 *)window.r0, (const float4 *)window.r1, window.kept.get(), call.gamma);
		}
		CTX_TRY(c, hipGetLastError());
		return ADYPT_OK;
	}
	void finished(const DenoiseCall &call) { if(call.history) valid = true; }
};

// following mirrors and glass (guide_chain.hpp): the chain's state, 32 B per local pixel, and its counters, allocated at the first call or guide
// read-out with bounces; the bounces of the last one (0: none has been enqueued) and the time of its chain stage.  It has no `valid` and no finished:
// its counters stay on the device, and fill reads them behind whatever the context's stream still holds.  enqueue: enqueue_chain below.
struct ChainStage {
	Buffer<float4> state;
	Buffer<ChainCounts> counts;
	int bounces = 0;
	StageTimer<2> timer;
	int ensure(adypt_ctx *c, size_t n_local_px) { CTX_TRY(c, at_least(state, n_local_px * 2)); CTX_TRY(c, at_least(counts, 1)); return ADYPT_OK; }
	int fill(adypt_ctx *c, adypt_denoise_specular_info *out) const;
};

struct LastRun { bool history = false; int levels = 0; };

// Everything the denoiser keeps per context; parked in the context (ctx_attachment), freed by adypt_destroy (the context's device is current then).
struct Denoiser {
	int width = 0, height = 0;
	BlockImages own, merged; // the context's own blocks (allocated at the first call: the size never changes); several devices: all blocks, on the first
	// the filter's row-major images of the whole picture: 80 B + 12 B (the result) per image pixel
	Buffer<float4> x0[2], x1, x2, xa;
	Buffer<float> rgb;
	StageTimer<kDenoiseTimingEvents> timer; // completed: the last filter ran to its end, rgb is its result and `last` says what it was
	LastRun last;
	History history; // allocated at the first call with history
	MergeStage merge;
	MotionStage motion;
	WindowStage window;
	MomentsStage moments;
	VirtualStage virt;
	ChainStage chain;

	size_t pixels() const { return (size_t)width * (size_t)height; }
	// room for what the call's stages write (and for the history they read); their read-outs are invalid from here until the call is finished
	int ensure_stages(adypt_ctx *c, const DenoiseCall &call)
	{
		const size_t n = pixels();
		if(call.history) { CTX_STEP(merge.ensure(c, n)); CTX_STEP(history.ensure(c, n)); }
		if(call.motion) CTX_STEP(motion.ensure(c, n));
		if(call.rectify) CTX_STEP(window.ensure(c, n));
		if(call.moments) CTX_STEP(moments.ensure(c, n));
		if(call.virtual_point()) CTX_STEP(virt.ensure(c, n));
		return ADYPT_OK;
	}
	// the call's stream has been waited for
	void finished(const DenoiseCall &call)
	{
		last = LastRun{call.history, call.prm.levels};
		timer.complete();
		merge.finished(call); motion.finished(call); window.finished(call); moments.finished(call); virt.finished(call);
	}
};

Denoiser *denoiser_of(adypt_ctx *c) { return ctx_state<Denoiser>(c, kAttachDenoise); }
Denoiser *finished_denoiser(adypt_ctx *c) { Denoiser *d = ctx_state_if_any<Denoiser>(c, kAttachDenoise); return d && d->timer.completed() ? d : nullptr; }

int ensure_filter_images(adypt_ctx *c, Denoiser *d, const CtxInfo &i)
{
	d->width = i.width; d->height = i.height;
	const size_t n = d->pixels();
	CTX_TRY(c, at_least(d->x0[0], n)); CTX_TRY(c, at_least(d->x0[1], n)); CTX_TRY(c, at_least(d->x1, n)); CTX_TRY(c, at_least(d->x2, n)); CTX_TRY(c, at_least(d->xa, n));
	CTX_TRY(c, at_least(d->rgb, n * 3));
	return ADYPT_OK;
}

// The steps of a call on `stream`, none of which waits for the host until the end; d's images are the whole picture's (ensure_filter_images), `cam`
// the camera of the context the guides were captured by.  A step in brackets is a stage only some calls have.
int run_filter(adypt_ctx *c, Denoiser *d, hipStream_t stream, const LocalImages &in, const DenoiseCall &call, const CtxCamera &cam)
{
	History &h = d->history;
	CTX_STEP(d->ensure_stages(c, call));
	const Picture px{d->x0[0].get(), d->x1.get(), d->x2.get(), d->xa.get(), d->width, d->height};
	const RectifyOrigin origin{{cam.origin[0], cam.origin[1], cam.origin[2]}};
	const int n_px = in.n_blocks * kBlockPixels;
	// prepare (followed guides: X1.w is the class the chain left in the .w of the primary-hit image; by the virtual point: XV beside the four)
	const LaunchShape prepare = prepare_launch(n_px);
	if(call.virtual_point())
		hipLaunchKernelGGL(k_denoise_prepare_virtual, prepare.grid, prepare.block, 0, stream, in.as<kAccum>(), in.as<kMoments>(), in.as<kBlocks>(), in.as<kBlockSpp>(), n_px, px.blocks_x(), px.width, px.height,
		                   in.as<kAlbedo>(), in.as<kNormal>(), in.as<kPosition>(), in.as<kHits>(), px.x0, px.x1, px.x2, px.xa, in.as<kVirtual>(), d->virt.xv.get());
	else
		hipLaunchKernelGGL(prepare_instance(call.moments, call.bounces > 0), prepare.grid, prepare.block, 0, stream, in.as<kAccum>(), in.as<kMoments>(), in.as<kBlocks>(), in.as<kBlockSpp>(), n_px, px.blocks_x(),
		                   px.width, px.height, in.as<kAlbedo>(), in.as<kNormal>(), in.as<kPosition>(), in.as<kHits>(), px.x0, px.x1, px.x2, px.xa);
	CTX_TRY(c, hipGetLastError());
	CTX_TRY(c, d->timer.mark(2, stream));
	const StageMarks marks = call.marks();
	if(call.history)
	{
		if(call.motion) CTX_STEP(d->motion.enqueue(c, stream, in, px, h));                           // [gather]
		if(call.rectify) CTX_STEP(d->window.enqueue(c, stream, px, origin, call));                   // [window]
		CTX_STEP(d->merge.enqueue(c, stream, px, h, call, d->motion, d->window, d->virt));           // merge
		if(call.moments) CTX_STEP(d->moments.enqueue(c, stream, px, d->merge.xm.get(), origin));     // [variance]
		CTX_TRY(c, d->timer.mark(marks.merge, stream));
	}
	const LaunchShape level_shape = atrous_launch(px.width, px.height);
	const DenoiseParams &prm = call.prm;
	for(int l = 0; l < prm.levels; ++l)
	{
		const float4 *src = l == 0 && call.levels_read_merged() ? d->merge.xm : d->x0[l & 1];
		float4 *dst = d->x0[(l & 1) ^ 1];
		hipLaunchKernelGGL(atrous_instance(l == prm.levels - 1), level_shape.grid, level_shape.block, 0, stream, src, (const float4 *)px.x1, (const float4 *)px.x2, (const float4 *)px.xa, dst, d->rgb.get(), px.width, px.height, 1 << l, prm.sigma_l, prm.sigma_z);
		CTX_TRY(c, hipGetLastError());
		CTX_TRY(c, d->timer.mark(marks.first_level + l, stream));
	}
	int64_t snapshot_of = 0;
	if(call.motion && call.commit) CTX_STEP(h.enqueue_snapshot(c, stream, &snapshot_of));            // [snapshot]
	CTX_TRY(c, hipStreamSynchronize(stream));
	d->finished(call);
	if(call.commit) h.commit(d->merge.xm, d->x1, d->x2, d->xa, cam, snapshot_of, call.kind());
	return ADYPT_OK;
}

// The stage times of the last finished run.  ms, where `capacity` holds them: guides, prepare and every level, adypt_get_denoise_timing's layout
// with or without history (returns their number); merge_ms, where not null: the merge's stage, which stands between prepare's and the first level's.
int read_stages(const Denoiser *d, float *ms, int capacity, float *merge_ms)
{
	const StageMarks marks = stage_marks(d->last.history);
	const int n = 2 + d->last.levels;
	float all[kDenoiseTimingEvents];
	d->timer.read(all, kDenoiseTimingEvents, marks.first_level - 1 + d->last.levels, false);
	if(merge_ms) *merge_ms = marks.merge ? all[marks.merge - 1] : 0.0f;
	if(capacity < n) return n;
	for(int k = 0; k < n; ++k) ms[k] = all[k < 2 ? k : k + marks.first_level - 3];
	return n;
}

// the context's own set, for `in` = ctx_denoise_inputs(c): the kContextImages are the context's (moments null while it keeps no noise statistics, which
// only the guide read-out goes without), the guides and the sample counts the denoiser's; left_out: optional_images of the call
int own_images(adypt_ctx *c, Denoiser *d, const DenoiseInputs &in, LocalImages *v, unsigned left_out = kWithoutVirtual)
{
	*v = LocalImages{{}, in.n_blocks};
	v->image[kAccum] = in.accum; v->image[kMoments] = in.moments; v->image[kBlocks] = in.blocks;
	return d->own.fill(c, v, kContextImages | left_out);
}

// The chain through mirrors and glass over the context's own blocks (guide_chain.hpp), enqueued behind the guide capture on the context's stream
// without a host sync: k_chain_start, then `bounces` rounds of the context's k_trace over the queue just written and k_chain_step, which writes the
// other queue.  Every round is enqueued whether it has rays or not: an empty round measures 0.05 ms (two launches that read eight counters), and
// stopping at the first one would need a count read back — a host sync in a call that has none until its end (that form is not built).
// The queues have been asked for (ctx_ray_queues) before the capture was enqueued.
// Where the set `own` has room for virtual points (a call by the virtual point: optional_images) the unfolding instances run, which also leave them
// there (the same queues, segments and capacity check).
int enqueue_chain(adypt_ctx *c, Denoiser *d, const DenoiseInputs &in, const char *fn, int bounces, const CtxRayQueues &q, const LocalImages &own)
{
	const CtxInfo i = ctx_info(c);
	const int n_px = in.n_blocks * kBlockPixels;
	const LaunchShape start = chain_start_launch(n_px);
	const uint32_t per_segment = ((start.grid.x + (unsigned)q.segments - 1) / (unsigned)q.segments) * kPixelThreads; // the most rays a segment is given
	if(per_segment > q.seg_cap || bounces + 1 > q.rounds) return ctx_fail(c, ADYPT_E_STATE, std::string(fn) + ": the context's ray queues cannot hold the chain's rays");
	ChainStage &chain = d->chain;
	CTX_STEP(chain.ensure(c, (size_t)n_px));
	const CtxScene scene = ctx_scene(c);
	const CtxMaterials mats = ctx_materials(c);
	const CtxCamera cam = ctx_camera(c);
	const ChainScene sc{(const float4 *)scene.triangles, mats.materials, mats.texels, scene.n_tris, (int32_t)mats.n_mats, mats.n_textures};
	const ChainGuides g{d->own.as<kAlbedo>(), d->own.as<kNormal>(), d->own.as<kPosition>(), d->own.as<kHits>()};
	const ChainOrigin origin{{cam.origin[0], cam.origin[1], cam.origin[2]}, q.tmin};
	auto queue = [&q](int parity, int round) { return ChainQueue{q.o[parity], q.d[parity], q.count + (size_t)round * q.round_stride, q.seg_cap, q.seg_stride, q.segments}; };
	const int blocks_x = (i.width + kBlockDim - 1) / kBlockDim;
	const bool unfold = own.image[kVirtual] != nullptr;
	chain.bounces = bounces;
	CTX_TRY(c, hipMemsetAsync(chain.counts.get(), 0, sizeof(ChainCounts), i.stream));
	CTX_TRY(c, chain.timer.mark(0, i.stream));
	hipLaunchKernelGGL(chain_start_instance(unfold), start.grid, start.block, 0, i.stream, sc, g, in.blocks, n_px, blocks_x, i.width, i.height, origin, bounces, chain.state.get(), queue(0, 0),
	                   chain.counts.get());
	const ChainUnfold unfolded{unfold ? d->own.as<kVirtual>() : nullptr, {cam.origin[0], cam.origin[1], cam.origin[2]}};
	CTX_TRY(c, hipGetLastError());
	const LaunchShape step = chain_step_launch(q.segments, per_segment);
	for(int r = 0; r < bounces; ++r)
	{
		CTX_STEP(ctx_trace_queue(c, r & 1, r));
		hipLaunchKernelGGL(chain_step_instance(unfold), step.grid, step.block, 0, i.stream, sc, g, queue(r & 1, r), (const float4 *)q.hit, n_px, bounces, q.tmin, chain.state.get(),
		                   queue((r & 1) ^ 1, r + 1), chain.counts.get(), unfolded);
		CTX_TRY(c, hipGetLastError());
	}
	CTX_TRY(c, chain.timer.mark(1, i.stream));
	return ADYPT_OK;
}

// ... and the context's guides into it, enqueued behind its frames (the sample counts are the caller's to upload); bounces > 0: followed through mirrors
// and glass, the class of every pixel in the .w of the primary-hit image
int capture_guides(adypt_ctx *c, Denoiser *d, const DenoiseInputs &in, const char *fn, LocalImages *v, int bounces = 0, unsigned left_out = kWithoutVirtual)
{
	CTX_STEP(own_images(c, d, in, v, left_out));
	CtxRayQueues q{};
	if(bounces > 0) CTX_STEP(ctx_ray_queues(c, fn, &q)); // (first: it may have to wait for frames started ahead)
	CTX_STEP(ctx_capture_guides(c, fn, d->own.as<kAlbedo>(), d->own.as<kNormal>(), d->own.as<kPosition>(), d->own.as<kHits>()));
	return bounces > 0 && in.n_blocks > 0 ? enqueue_chain(c, d, in, fn, bounces, q, *v) : (int)ADYPT_OK;
}

// `bytes` of a device array of a context on the host (the stream is drained when it returns)
int fetch(adypt_ctx *c, const CtxInfo &i, const void *device, void *host, size_t bytes)
{
	CTX_TRY(c, hipMemcpyAsync(host, device, bytes, hipMemcpyDeviceToHost, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	return ADYPT_OK;
}

// A read-out of an image of the last finished run, per_pixel elements per image pixel: `image` picks it, null where the denoiser has none to read, and
// the call is then refused with `none`.
template <class T, class Pick> int read_image(adypt_ctx *c, const char *fn, const char *none, T *host, int per_pixel, Pick image)
{
	Denoiser *d = finished_denoiser(c);
	const T *device = d ? image(d) : nullptr;
	if(!device) return ctx_fail(c, ADYPT_E_STATE, std::string(fn) + none);
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	return fetch(c, i, device, host, d->pixels() * per_pixel * sizeof(T));
}

int read_result(adypt_ctx *c, const char *fn, float *rgb)
{
	return read_image(c, fn, ": nothing has been denoised yet (adypt_denoise)", rgb, 3, [](Denoiser *d) { return d->rgb.get(); });
}

int read_history_length(adypt_ctx *c, const char *fn, float *length)
{
	return read_image(c, fn, ": no temporal call has run yet (adypt_denoise_temporal)", length, 1, [](Denoiser *d) { return d->merge.valid ? d->merge.length.get() : nullptr; });
}

// A float4 read-out image of the last finished run (`image` as read_image's) split into the caller's arrays: xyz, W x H x 3 floats, and w through
// `flag`, W x H elements; either may be null
template <class W, class Pick, class Flag> int read_split(adypt_ctx *c, const char *fn, const char *none, float *xyz, W *w, Pick image, Flag flag)
{
	Denoiser *d = finished_denoiser(c);
	std::vector<float4> host(d && image(d) ? d->pixels() : 0); // (nothing where the call is about to be refused)
	CTX_STEP(read_image(c, fn, none, host.data(), 1, image));
	for(size_t k = 0; k < host.size(); ++k)
	{
		if(xyz) { xyz[3 * k] = host[k].x; xyz[3 * k + 1] = host[k].y; xyz[3 * k + 2] = host[k].z; }
		if(w) w[k] = flag(host[k].w);
	}
	return ADYPT_OK;
}

// XP of the last motion call: the previous position and the moved flag (bytes) of every pixel
int read_motion(adypt_ctx *c, const char *fn, float *prev_position, uint8_t *moved)
{
	return read_split(c, fn, ": no motion call has run yet (adypt_denoise_temporal_motion)", prev_position, moved, [](Denoiser *d) { return d->motion.valid ? d->motion.xp.get() : nullptr; },
	                  [](float w) { return (uint8_t)(w != 0.0f ? 1 : 0); });
}

// XV of the last call by the virtual point: the virtual position and the unfolded length (0: the pixel is not followed, or its length is not valid)
int read_virtual(adypt_ctx *c, const char *fn, float *virtual_position, float *distance)
{
	return read_split(c, fn, ": no call by the virtual point has run yet (adypt_denoise_temporal_specular)", virtual_position, distance,
	                  [](Denoiser *d) { return d->virt.valid ? d->virt.xv.get() : nullptr; }, [](float w) { return w; });
}

// the share of its length every pixel's history kept in the last rectified call
int read_rectify(adypt_ctx *c, const char *fn, float *kept)
{
	return read_image(c, fn, ": no rectified call has run yet (adypt_denoise_temporal_rectified)", kept, 1, [](Denoiser *d) { return d->window.valid ? d->window.kept.get() : nullptr; });
}

// the variance the first level saw in the last moments call
int read_variance(adypt_ctx *c, const char *fn, float *v)
{
	return read_image(c, fn, ": no moments call has run yet (adypt_denoise_temporal_moments)", v, 1, [](Denoiser *d) { return d->moments.valid ? d->moments.variance.get() : nullptr; });
}

// What an adypt_get_denoise_* call answers: `out` refused when null, zeroed, and — where the context has denoised at all — filled by `fill`
// (an int: ADYPT_OK, or the step that failed)
template <class Info, class Fill> int get_info(adypt_ctx *c, const char *fn, Info *out, Fill fill)
{
	if(!out) return ctx_fail(c, ADYPT_E_INVALID, std::string(fn) + ": out is null");
	*out = Info{};
	const Denoiser *d = ctx_state_if_any<Denoiser>(c, kAttachDenoise);
	return d ? fill(d) : (int)ADYPT_OK;
}

int get_motion(adypt_ctx *c, const char *fn, adypt_denoise_motion *out)
{
	return get_info(c, fn, out, [out](const Denoiser *d) { d->motion.fill(d->history, out); return (int)ADYPT_OK; });
}

int get_rectify(adypt_ctx *c, const char *fn, adypt_denoise_rectify *out)
{
	return get_info(c, fn, out, [out](const Denoiser *d) { d->window.fill(out); return (int)ADYPT_OK; });
}

int get_moments(adypt_ctx *c, const char *fn, adypt_denoise_moments *out)
{
	return get_info(c, fn, out, [out](const Denoiser *d) { d->moments.fill(out); return (int)ADYPT_OK; });
}

int get_virtual(adypt_ctx *c, const char *fn, adypt_denoise_virtual *out)
{
	return get_info(c, fn, out, [out](const Denoiser *d) { d->virt.fill(d->own.image[kVirtual].bytes() + d->merged.image[kVirtual].bytes(), out); return (int)ADYPT_OK; });
}

int read_guides(adypt_ctx *c, const char *fn, int bounces, float *albedo, float *normal, float *position, uint8_t *hit, int8_t *chain); // (below, beside its entry points)

// what the last chain of a context did: its counters are read here, behind whatever the context's stream still holds
int ChainStage::fill(adypt_ctx *c, adypt_denoise_specular_info *out) const
{
	out->device_bytes = (int64_t)(state.bytes() + counts.bytes());
	if(bounces == 0) return ADYPT_OK;
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	ChainCounts n;
	CTX_STEP(fetch(c, i, counts.get(), &n, sizeof(n)));
	out->have = 1; out->bounces = bounces;
	(void)timer.read(&out->chain_ms, 1, 1, false);
	out->rays = (int64_t)n.rays; out->pixels_followed = (int64_t)n.followed; out->pixels_escaped = (int64_t)n.escaped; out->pixels_truncated = (int64_t)n.truncated;
	return ADYPT_OK;
}

int get_specular(adypt_ctx *c, const char *fn, adypt_denoise_specular_info *out)
{
	return get_info(c, fn, out, [c, out](const Denoiser *d) { return d->chain.fill(c, out); });
}

int read_merge_ms(adypt_ctx *c, const char *fn, float *ms)
{
	Denoiser *d = finished_denoiser(c);
	if(!d || !d->last.history) return ctx_fail(c, ADYPT_E_STATE, std::string(fn) + ": the last filter was not a temporal call (adypt_denoise_temporal)");
	read_stages(d, nullptr, 0, ms);
	return ADYPT_OK;
}

// a denoise call of one context
int denoise_context(adypt_ctx *c, const DenoiseCall &call)
{
	if(!c) return ADYPT_E_INVALID;
	if(!call.refused.empty()) return ctx_fail(c, ADYPT_E_INVALID, call.refused);
	const char *fn = call.fn;
	const CtxInfo i = ctx_info(c);
	if(i.nranks != 1) return ctx_fail(c, ADYPT_E_STATE, std::string(fn) + ": the context is a tile shard (tile_nranks > 1): the filter needs the whole image (adypt_multi_denoise)");
	CTX_STEP(ctx_denoise_ready(c, fn, call.min_spp()));
	CTX_TRY(c, hipSetDevice(i.device));
	Denoiser *d = denoiser_of(c);
	CTX_STEP(ensure_filter_images(c, d, i));
	d->timer.invalidate();
	CTX_TRY(c, d->timer.mark(0, i.stream));
	const DenoiseInputs in = ctx_denoise_inputs(c);
	LocalImages local;
	CTX_STEP(capture_guides(c, d, in, fn, &local, call.bounces, optional_images(call)));
	CTX_TRY(c, d->timer.mark(1, i.stream));
	CTX_TRY(c, hipMemcpyAsync(d->own.as<kBlockSpp>(), in.block_spp.data(), in.block_spp.size() * sizeof(int32_t), hipMemcpyHostToDevice, i.stream));
	return run_filter(c, d, i.stream, local, call, ctx_camera(c));
}

}  // namespace

namespace adypt {

void denoise_triangles_replaced(adypt_ctx *c)
{
	if(Denoiser *d = ctx_state_if_any<Denoiser>(c, kAttachDenoise)) d->history.triangles_replaced();
}

}  // namespace adypt

extern "C" {

int adypt_denoise(adypt_ctx *c, const adypt_denoise_params *p) { return denoise_context(c, make_call("adypt_denoise", 0, p)); }

int adypt_denoise_temporal(adypt_ctx *c, const adypt_denoise_params *p, const adypt_temporal_params *tp) { return denoise_context(c, make_call("adypt_denoise_temporal", kWithHistory, p, tp)); }

int adypt_denoise_temporal_motion(adypt_ctx *c, const adypt_denoise_params *p, const adypt_temporal_params *tp) { return denoise_context(c, make_call("adypt_denoise_temporal_motion", kWithHistory | kWithMotion, p, tp)); }

int adypt_denoise_temporal_rectified(adypt_ctx *c, const adypt_denoise_params *p, const adypt_temporal_params *tp, const adypt_rectify_params *rp, int follow_motion)
{
	return denoise_context(c, make_call("adypt_denoise_temporal_rectified", kWithHistory | kWithRectify | motion_if(follow_motion), p, tp, rp));
}

int adypt_denoise_temporal_moments(adypt_ctx *c, const adypt_denoise_params *p, const adypt_temporal_params *tp, int follow_motion)
{
	return denoise_context(c, make_call("adypt_denoise_temporal_moments", kWithHistory | kWithMoments | motion_if(follow_motion), p, tp));
}

int adypt_read_denoise_variance(adypt_ctx *c, float *v) { return c && v ? read_variance(c, "adypt_read_denoise_variance", v) : ADYPT_E_INVALID; }

int adypt_get_denoise_moments(adypt_ctx *c, adypt_denoise_moments *out) { return c ? get_moments(c, "adypt_get_denoise_moments", out) : ADYPT_E_INVALID; }

int adypt_read_denoise_rectify(adypt_ctx *c, float *kept) { return c && kept ? read_rectify(c, "adypt_read_denoise_rectify", kept) : ADYPT_E_INVALID; }

int adypt_get_denoise_rectify(adypt_ctx *c, adypt_denoise_rectify *out) { return c ? get_rectify(c, "adypt_get_denoise_rectify", out) : ADYPT_E_INVALID; }

int adypt_denoise_history_reset(adypt_ctx *c)
{
	if(!c) return ADYPT_E_INVALID;
	if(Denoiser *d = ctx_state_if_any<Denoiser>(c, kAttachDenoise)) d->history.reset();
	return ADYPT_OK;
}

int adypt_read_denoise_motion(adypt_ctx *c, float *prev_position, uint8_t *moved) { return c ? read_motion(c, "adypt_read_denoise_motion", prev_position, moved) : ADYPT_E_INVALID; }

int adypt_get_denoise_motion(adypt_ctx *c, adypt_denoise_motion *out) { return c ? get_motion(c, "adypt_get_denoise_motion", out) : ADYPT_E_INVALID; }

int adypt_read_denoise_history(adypt_ctx *c, float *length) { return c && length ? read_history_length(c, "adypt_read_denoise_history", length) : ADYPT_E_INVALID; }

int adypt_get_denoise_merge_ms(adypt_ctx *c, float *ms) { return c && ms ? read_merge_ms(c, "adypt_get_denoise_merge_ms", ms) : ADYPT_E_INVALID; }

int adypt_read_denoised(adypt_ctx *c, float *rgb) { return c && rgb ? read_result(c, "adypt_read_denoised", rgb) : ADYPT_E_INVALID; }

int adypt_read_denoise_guides(adypt_ctx *c, float *albedo, float *normal, float *position, uint8_t *hit)
{
	return c ? read_guides(c, "adypt_read_denoise_guides", 0, albedo, normal, position, hit, nullptr) : ADYPT_E_INVALID;
}

int adypt_read_denoise_guides_specular(adypt_ctx *c, int32_t bounces, float *albedo, float *normal, float *position, int8_t *chain)
{
	if(!c) return ADYPT_E_INVALID;
	if(!chain_bounces_valid(bounces)) return ctx_fail(c, ADYPT_E_INVALID, "adypt_read_denoise_guides_specular: bounces must be in [1, " + std::to_string(kChainMaxBounces) + "]");
	return read_guides(c, "adypt_read_denoise_guides_specular", bounces, albedo, normal, position, nullptr, chain);
}

int adypt_denoise_specular(adypt_ctx *c, const adypt_denoise_params *p, const adypt_specular_params *sp) { return denoise_context(c, make_call("adypt_denoise_specular", kWithSpecular, p, nullptr, nullptr, sp)); }

int adypt_get_denoise_specular(adypt_ctx *c, adypt_denoise_specular_info *out) { return c ? get_specular(c, "adypt_get_denoise_specular", out) : ADYPT_E_INVALID; }

int adypt_denoise_temporal_specular(adypt_ctx *c, const adypt_denoise_params *p, const adypt_temporal_params *tp, const adypt_specular_params *sp)
{
	return denoise_context(c, make_call("adypt_denoise_temporal_specular", kWithHistory | kWithSpecular, p, tp, nullptr, sp));
}

int adypt_read_denoise_virtual(adypt_ctx *c, float *virtual_position, float *distance) { return c ? read_virtual(c, "adypt_read_denoise_virtual", virtual_position, distance) : ADYPT_E_INVALID; }

int adypt_get_denoise_virtual(adypt_ctx *c, adypt_denoise_virtual *out) { return c ? get_virtual(c, "adypt_get_denoise_virtual", out) : ADYPT_E_INVALID; }

}  // extern "C"

namespace {

// the guide read-out of a context: the pixels of its own blocks into the caller's images; bounces > 0: the followed guides, and `chain` the class codes
int read_guides(adypt_ctx *c, const char *fn, int bounces, float *albedo, float *normal, float *position, uint8_t *hit, int8_t *chain)
{
	const CtxInfo i = ctx_info(c);
	if(i.n_local_px == 0) return ADYPT_OK; // a shard that owns no block
	CTX_TRY(c, hipSetDevice(i.device));
	LocalImages own;
	CTX_STEP(capture_guides(c, denoiser_of(c), ctx_denoise_inputs(c), fn, &own, bounces));
	const std::vector<int32_t> blocks = owned_blocks(i.width, i.height, i.rank, i.nranks);
	std::vector<float4> local((size_t)i.n_local_px);
	float *const image[3] = {albedo, normal, position};
	const BlockImage guide[3] = {kAlbedo, kNormal, kPosition};
	for(int k = 0; k < 3; ++k)
	{
		if(!image[k]) continue;
		CTX_STEP(fetch(c, i, own.image[guide[k]], local.data(), local.size() * sizeof(float4)));
		for_each_local_pixel(blocks, i.width, i.height, [&](size_t L, int x, int y) {
			float *o = image[k] + ((size_t)y * i.width + x) * 3;
			o[0] = local[L].x; o[1] = local[L].y; o[2] = local[L].z;
		});
	}
	if(hit || chain)
	{
		CTX_STEP(fetch(c, i, own.image[kHits], local.data(), local.size() * sizeof(float4)));
		for_each_local_pixel(blocks, i.width, i.height, [&](size_t L, int x, int y) {
			int32_t tri;
			memcpy(&tri, &local[L].x, 4);
			if(hit) hit[(size_t)y * i.width + x] = tri != -1 ? 1 : 0;
			if(chain) chain[(size_t)y * i.width + x] = (int8_t)local[L].w;
		});
	}
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	return ADYPT_OK;
}

}  // namespace

extern "C" {

int adypt_get_denoise_timing(adypt_ctx *c, float *ms, int capacity)
{
	if(!c || !ms || capacity < 0) return ADYPT_E_INVALID;
	Denoiser *d = finished_denoiser(c);
	if(!d) return ctx_fail(c, ADYPT_E_STATE, "adypt_get_denoise_timing: nothing has been denoised yet (adypt_denoise)");
	return read_stages(d, ms, capacity, nullptr); // (a temporal call's merge stage is left out: adypt_get_denoise_merge_ms)
}

// ---- one process, N devices ----
}  // extern "C"

namespace {

// The first half of a call over several devices, which multi_denoise and the plan by history (denoise_plan_inputs_multi) share: every device
// captures the guides of its own blocks — all enqueued before the first is waited for; bounces > 0: every device follows the chains of its own
// blocks, the class comes along in the primary-hit image — and the host collects the local images of every device back to back in rank order, their
// block lists and sample counts likewise (the counts from each context's own state in that order: multi.hip's merge is sorted by block index, which
// is not this order, and would launch k_noise_blocks for nothing).  left_out: the images that neither travel nor are allocated.
struct HostImages { std::vector<uint8_t> image[kBlockImages]; size_t n_blocks = 0; };
int collect_guides(adypt_multi *m, const std::vector<adypt_ctx *> &ctx, const char *fn, int bounces, unsigned left_out, HostImages *out)
{
	auto fail_ctx = [m](adypt_ctx *c, int r) { multi_set_error(m, adypt_last_error(c)); return r; };
	CTX_STEP(multi_each(m, [fn, bounces, left_out](adypt_ctx *c) {
		const CtxInfo i = ctx_info(c);
		if(i.n_local_px == 0) return (int)ADYPT_OK;
		if(hipSetDevice(i.device) != hipSuccess) return ctx_fail(c, ADYPT_E_HIP, std::string(fn) + ": hipSetDevice failed");
		LocalImages own;
		return capture_guides(c, denoiser_of(c), ctx_denoise_inputs(c), fn, &own, bounces, left_out);
	}));
	size_t n_blocks = 0;
	for(adypt_ctx *c : ctx) n_blocks += (size_t)ctx_info(c).n_local_px / kBlockPixels;
	std::vector<uint8_t> *host = out->image;
	for(int k = 0; k < kBlockImages; ++k)
		if(!(left_out >> k & 1)) host[k].resize(n_blocks * kBlockImageBytes[k]);
	size_t at = 0; // the rank's first block in them
	for(adypt_ctx *c : ctx)
	{
		const CtxInfo i = ctx_info(c);
		if(i.n_local_px == 0) continue;
		if(hipSetDevice(i.device) != hipSuccess) return fail_ctx(c, ctx_fail(c, ADYPT_E_HIP, std::string(fn) + ": hipSetDevice failed"));
		const DenoiseInputs in = ctx_denoise_inputs(c);
		LocalImages own;
		int r = own_images(c, denoiser_of(c), in, &own, left_out);
		for(const BlockImage k : kFetchOrder)
			if(r == ADYPT_OK && !(left_out >> k & 1)) r = fetch(c, i, own.image[k], host[k].data() + at * kBlockImageBytes[k], (size_t)in.n_blocks * kBlockImageBytes[k]);
		if(r != ADYPT_OK) return fail_ctx(c, r);
		memcpy(host[kBlocks].data() + at * sizeof(int32_t), in.block_index.data(), in.block_index.size() * sizeof(int32_t));
		if(!(left_out >> kBlockSpp & 1)) memcpy(host[kBlockSpp].data() + at * sizeof(int32_t), in.block_spp.data(), in.block_spp.size() * sizeof(int32_t));
		at += (size_t)in.n_blocks;
	}
	out->n_blocks = n_blocks;
	return ADYPT_OK;
}
// ... uploaded to the set `merged` of the first device, whose device is current: enqueued on `stream`, `host` has to outlive the wait for it
int upload_guides(adypt_ctx *c, Denoiser *d, hipStream_t stream, const HostImages &host, unsigned left_out)
{
	for(int k = 0; k < kBlockImages; ++k)
		if(!(left_out >> k & 1)) CTX_TRY(c, hipMemcpyAsync(d->merged.image[k], host.image[k].data(), host.image[k].size(), hipMemcpyHostToDevice, stream));
	return ADYPT_OK;
}

// a denoise call of a handle: the merge runs on the first device, where the filter runs, and the history lives there
int multi_denoise(adypt_multi *m, const DenoiseCall &call)
{
	const int n_dev = adypt_multi_device_count(m);
	if(n_dev < 1) return ADYPT_E_INVALID;
	adypt_ctx *root = adypt_multi_context(m, 0);
	if(n_dev == 1) return multi_each(m, [&call](adypt_ctx *c) { return denoise_context(c, call); });
	auto fail_ctx = [m](adypt_ctx *c, int r) { multi_set_error(m, adypt_last_error(c)); return r; };
	if(!call.refused.empty()) { multi_set_error(m, call.refused); return ADYPT_E_INVALID; }
	const char *fn = call.fn;
	std::vector<adypt_ctx *> ctx;
	for(int k = 0; k < n_dev; ++k) ctx.push_back(adypt_multi_context(m, k));
	const int min_spp = call.min_spp();
	CTX_STEP(multi_each(m, [fn, min_spp](adypt_ctx *c) { return ctx_denoise_ready(c, fn, min_spp); }));
	const unsigned left_out = optional_images(call);
	HostImages host;
	CTX_STEP(collect_guides(m, ctx, fn, call.bounces, left_out, &host));
	const CtxInfo ri = ctx_info(root);
	const size_t n_blocks = host.n_blocks;
	// ... uploaded to the first device, where the same prepare / a-trous launches run
	adypt_ctx *c = root;
	auto steps = [&]() -> int {
		CTX_TRY(c, hipSetDevice(ri.device));
		Denoiser *d = denoiser_of(c);
		CTX_STEP(ensure_filter_images(c, d, ri));
		d->timer.invalidate();
		LocalImages all{{}, (int)n_blocks};
		CTX_STEP(d->merged.fill(c, &all, left_out)); // (it borrows none)
		CTX_TRY(c, d->timer.mark(0, ri.stream));
		CTX_STEP(upload_guides(c, d, ri.stream, host, left_out));
		CTX_TRY(c, d->timer.mark(1, ri.stream));
		return run_filter(c, d, ri.stream, all, call, ctx_camera(c)); // (adypt_multi_set_camera gives every context the same camera)
	};
	const int r = steps();
	return r == ADYPT_OK ? r : fail_ctx(root, r);
}

// a per-context call on the first device's context, its error becoming the handle's
template <class F> int on_root(adypt_multi *m, F f)
{
	if(adypt_multi_device_count(m) < 1) return ADYPT_E_INVALID;
	adypt_ctx *root = adypt_multi_context(m, 0);
	const int r = f(root);
	if(r != ADYPT_OK) multi_set_error(m, adypt_last_error(root));
	return r;
}

// a per-device info struct over the devices: every device's bytes, and `add` for what the devices that have something say
template <class Info, class Get, class Add> int sum_info(adypt_multi *m, Info *out, Get get, Add add)
{
	if(!out) return ADYPT_E_INVALID;
	Info sum{};
	const int r = multi_each(m, [&](adypt_ctx *c) {
		Info one;
		const int e = get(c, &one);
		if(e != ADYPT_OK) return e;
		sum.device_bytes += one.device_bytes;
		if(one.have) { sum.have = 1; sum.bounces = one.bounces; add(&sum, one); }
		return (int)ADYPT_OK;
	});
	if(r == ADYPT_OK) *out = sum;
	return r;
}

}  // namespace

extern "C" {

int adypt_multi_denoise(adypt_multi *m, const adypt_denoise_params *p) { return multi_denoise(m, make_call("adypt_multi_denoise", 0, p)); }

int adypt_multi_denoise_temporal(adypt_multi *m, const adypt_denoise_params *p, const adypt_temporal_params *tp) { return multi_denoise(m, make_call("adypt_multi_denoise_temporal", kWithHistory, p, tp)); }

int adypt_multi_denoise_temporal_motion(adypt_multi *m, const adypt_denoise_params *p, const adypt_temporal_params *tp) { return multi_denoise(m, make_call("adypt_multi_denoise_temporal_motion", kWithHistory | kWithMotion, p, tp)); }

int adypt_multi_denoise_temporal_rectified(adypt_multi *m, const adypt_denoise_params *p, const adypt_temporal_params *tp, const adypt_rectify_params *rp, int follow_motion)
{
	return multi_denoise(m, make_call("adypt_multi_denoise_temporal_rectified", kWithHistory | kWithRectify | motion_if(follow_motion), p, tp, rp));
}

int adypt_multi_denoise_temporal_moments(adypt_multi *m, const adypt_denoise_params *p, const adypt_temporal_params *tp, int follow_motion)
{
	return multi_denoise(m, make_call("adypt_multi_denoise_temporal_moments", kWithHistory | kWithMoments | motion_if(follow_motion), p, tp));
}

// the variance read-out and the count live on the first device, where the merge and the variance kernel run
int adypt_multi_read_denoise_variance(adypt_multi *m, float *v)
{
	return v ? on_root(m, [=](adypt_ctx *c) { return read_variance(c, "adypt_multi_read_denoise_variance", v); }) : ADYPT_E_INVALID;
}

int adypt_multi_get_denoise_moments(adypt_multi *m, adypt_denoise_moments *out)
{
	return on_root(m, [=](adypt_ctx *c) { return get_moments(c, "adypt_multi_get_denoise_moments", out); });
}

// the window statistics and the kept read-out live on the first device, where the merge runs
int adypt_multi_read_denoise_rectify(adypt_multi *m, float *kept)
{
	return kept ? on_root(m, [=](adypt_ctx *c) { return read_rectify(c, "adypt_multi_read_denoise_rectify", kept); }) : ADYPT_E_INVALID;
}

int adypt_multi_get_denoise_rectify(adypt_multi *m, adypt_denoise_rectify *out)
{
	return on_root(m, [=](adypt_ctx *c) { return get_rectify(c, "adypt_multi_get_denoise_rectify", out); });
}

// the snapshot and the motion images live on the first device, beside the history
int adypt_multi_read_denoise_motion(adypt_multi *m, float *prev_position, uint8_t *moved)
{
	return on_root(m, [=](adypt_ctx *c) { return read_motion(c, "adypt_multi_read_denoise_motion", prev_position, moved); });
}

int adypt_multi_get_denoise_motion(adypt_multi *m, adypt_denoise_motion *out)
{
	return on_root(m, [=](adypt_ctx *c) { return get_motion(c, "adypt_multi_get_denoise_motion", out); });
}

int adypt_multi_denoise_history_reset(adypt_multi *m) { return on_root(m, [](adypt_ctx *c) { return adypt_denoise_history_reset(c); }); }

int adypt_multi_read_denoise_history(adypt_multi *m, float *length)
{
	return length ? on_root(m, [=](adypt_ctx *c) { return read_history_length(c, "adypt_multi_read_denoise_history", length); }) : ADYPT_E_INVALID;
}

int adypt_multi_get_denoise_merge_ms(adypt_multi *m, float *ms)
{
	return ms ? on_root(m, [=](adypt_ctx *c) { return read_merge_ms(c, "adypt_multi_get_denoise_merge_ms", ms); }) : ADYPT_E_INVALID;
}

int adypt_multi_read_denoised(adypt_multi *m, float *rgb)
{
	return rgb ? on_root(m, [=](adypt_ctx *c) { return read_result(c, "adypt_multi_read_denoised", rgb); }) : ADYPT_E_INVALID;
}

// every device writes the pixels of its own tiles
int adypt_multi_read_denoise_guides(adypt_multi *m, float *albedo, float *normal, float *position, uint8_t *hit)
{
	return multi_each(m, [=](adypt_ctx *c) { return adypt_read_denoise_guides(c, albedo, normal, position, hit); });
}

int adypt_multi_denoise_specular(adypt_multi *m, const adypt_denoise_params *p, const adypt_specular_params *sp) { return multi_denoise(m, make_call("adypt_multi_denoise_specular", kWithSpecular, p, nullptr, nullptr, sp)); }

int adypt_multi_denoise_temporal_specular(adypt_multi *m, const adypt_denoise_params *p, const adypt_temporal_params *tp, const adypt_specular_params *sp)
{
	return multi_denoise(m, make_call("adypt_multi_denoise_temporal_specular", kWithHistory | kWithSpecular, p, tp, nullptr, sp));
}

// XV and the counts live on the first device, where the merge runs; the bytes are summed over the devices (every device keeps its own blocks' virtual points)
int adypt_multi_read_denoise_virtual(adypt_multi *m, float *virtual_position, float *distance)
{
	return on_root(m, [=](adypt_ctx *c) { return read_virtual(c, "adypt_multi_read_denoise_virtual", virtual_position, distance); });
}

int adypt_multi_get_denoise_virtual(adypt_multi *m, adypt_denoise_virtual *out)
{
	return sum_info(m, out, [](adypt_ctx *c, adypt_denoise_virtual *one) { return get_virtual(c, "adypt_multi_get_denoise_virtual", one); },
	                [](adypt_denoise_virtual *sum, const adypt_denoise_virtual &one) { sum->pixels_followed = one.pixels_followed; sum->pixels_with_history = one.pixels_with_history; });
}

int adypt_multi_read_denoise_guides_specular(adypt_multi *m, int32_t bounces, float *albedo, float *normal, float *position, int8_t *chain)
{
	return multi_each(m, [=](adypt_ctx *c) { return adypt_read_denoise_guides_specular(c, bounces, albedo, normal, position, chain); });
}

// every device followed the chains of its own blocks: the counts and the bytes are sums, the time the slowest device's
int adypt_multi_get_denoise_specular(adypt_multi *m, adypt_denoise_specular_info *out)
{
	return sum_info(m, out, [](adypt_ctx *c, adypt_denoise_specular_info *one) { return get_specular(c, "adypt_multi_get_denoise_specular", one); },
	                [](adypt_denoise_specular_info *sum, const adypt_denoise_specular_info &one) {
		                sum->chain_ms = std::max(sum->chain_ms, one.chain_ms);
		                sum->rays += one.rays; sum->pixels_followed += one.pixels_followed; sum->pixels_escaped += one.pixels_escaped; sum->pixels_truncated += one.pixels_truncated;
	                });
}

}  // extern "C"

// ---- what history_plan.hip needs (denoise_internal.hpp) ----
namespace {

// the images a plan goes without: it is made at 0 spp, of the guides alone
constexpr unsigned kPlanLeftOut = kWithoutVirtual | 1u << kAccum | 1u << kMoments | 1u << kBlockSpp;

// the guides of the set `v` and the history a call of the kind {moments, 0} finds in d
void plan_inputs_of(adypt_ctx *c, const Denoiser *d, const LocalImages &v, bool moments, PlanInputs *out)
{
	const History &h = d->history;
	out->albedo = v.as<kAlbedo>(); out->normal = v.as<kNormal>(); out->position = v.as<kPosition>(); out->hits = v.as<kHits>();
	out->blocks = v.as<kBlocks>(); out->n_blocks = v.n_blocks;
	out->have = h.present && h.kind == HistoryKind{moments, 0} ? 1 : 0;
	out->h0 = h.h0; out->h1 = h.h1; out->h2 = h.h2; out->ha = h.ha;
	out->camera = h.camera;
	out->snapshot = h.snapshot;
	out->known_tris = h.known_tris(ctx_scene(c).n_tris);
}

}  // namespace

namespace adypt {

int denoise_plan_inputs(adypt_ctx *c, const char *fn, bool moments, PlanInputs *out)
{
	Denoiser *d = denoiser_of(c);
	const DenoiseInputs in = ctx_denoise_inputs(c);
	LocalImages local;
	CTX_STEP(capture_guides(c, d, in, fn, &local));
	plan_inputs_of(c, d, local, moments, out);
	out->block_index = in.block_index;
	return ADYPT_OK;
}

int denoise_plan_inputs_multi(adypt_multi *m, const char *fn, bool moments, PlanInputs *out)
{
	const int n_dev = adypt_multi_device_count(m);
	std::vector<adypt_ctx *> ctx;
	for(int k = 0; k < n_dev; ++k) ctx.push_back(adypt_multi_context(m, k));
	HostImages host;
	CTX_STEP(collect_guides(m, ctx, fn, 0, kPlanLeftOut, &host));
	adypt_ctx *c = ctx[0];
	const CtxInfo ri = ctx_info(c);
	auto steps = [&]() -> int {
		CTX_TRY(c, hipSetDevice(ri.device));
		Denoiser *d = denoiser_of(c);
		LocalImages all{{}, (int)host.n_blocks};
		CTX_STEP(d->merged.fill(c, &all, kPlanLeftOut));
		CTX_STEP(upload_guides(c, d, ri.stream, host, kPlanLeftOut));
		CTX_TRY(c, hipStreamSynchronize(ri.stream)); // (the host's copies end with this call)
		plan_inputs_of(c, d, all, moments, out);
		out->block_index.resize(host.n_blocks);
		memcpy(out->block_index.data(), host.image[kBlocks].data(), host.n_blocks * sizeof(int32_t));
		return ADYPT_OK;
	};
	const int r = steps();
	if(r != ADYPT_OK) multi_set_error(m, adypt_last_error(c));
	return r;
}

}  // namespace adypt
