// The denoiser (include/adypt_hip.h adypt_denoise ...; the definition: denoise.hpp).  A translation unit of its own: nothing here is part of the
// tracer's code object.  What runs, all on the context's stream behind the frames:
//     guide capture  three launches of the viewer instance of k_trace_camera over the owned blocks (tracer.hip ctx_capture_guides), into scratch
//                    owned here: albedo, normal, position, primary hit — block-major like every local image
//     k_denoise_prepare  block-major accum / moments / block sample counts / guides  ->  row-major float4 images X0 = (D0.rgb, V0), X1 = (N.xyz, hit),
//                    X2 = (P.xyz, n), XA = (A.rgb, .)
//     k_temporal_merge  adypt_denoise_temporal only (the definition: temporal.hpp): the history the last committing call left — its merged pre-filter
//                    (D, V), its guides, its effective sample counts, its camera — reprojected through P and merged into (D0, V0); the levels then
//                    read the merged image.  A commit swaps the call's images with the history's: nothing is copied
//     k_motion_gather  adypt_denoise_temporal_motion only, before the merge and inside its stage of the timer: per pixel the hit triangle's words 0..17
//                    as the last committing motion call left them (the snapshot) against the record as it is now -> where the hit point and its normal
//                    WERE then (temporal_previous_point), row-major XP = (P_prev.xyz, moved), XN = (N_prev.xyz, valid); k_temporal_merge<true> merges
//                    through them.  k_motion_snapshot, on such a call's commit: the first 80 bytes of every record into the snapshot
//     k_atrous<LAST>  one level per launch, X0 ping-pongs; the last level multiplies the albedo back and writes the W x H x 3 result
// Several devices: every context captures the guides of its own blocks, the host puts the devices' local images back to back in rank order, their
// block lists likewise (every block has one owner, and k_denoise_prepare takes any block list and writes at the picture's coordinates), uploads them
// to the first device and runs the same kernels there (the merge too: the history lives on the first device) — no collective; the result is the
// one-device result bit for bit because the inputs are.
#include "ctx_unit.hpp"
#include "tile_layout.hpp"
#include "denoise.hpp"
#include "temporal.hpp"
#include "denoise_internal.hpp"
#include "../../../include/adypt_hip.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace adypt;

namespace {

__global__ __launch_bounds__(256) void k_denoise_prepare(const float4 *accum, const float2 *moments, const int32_t *blocks, const int32_t *block_spp, int n_px, int blocks_x, int width,
                                                         int height, const float4 *g_albedo, const float4 *g_normal, const float4 *g_position, const float4 *g_hits, float4 *x0,
                                                         float4 *x1, float4 *x2, float4 *xa)
{
	const int L = blockIdx.x * blockDim.x + threadIdx.x;
	if(L >= n_px) return;
	int x, y;
	block_pixel_xy(blocks[L >> 10], L & 1023, blocks_x, &x, &y);
	if(x >= width || y >= height) return; // (blocks at the right and bottom edge stick out)
	const size_t p = (size_t)y * width + x;
	const float4 c = accum[L], a = g_albedo[L], n = g_normal[L], q = g_position[L];
	const Dn4 d = denoise_prepare(c.x, c.y, c.z, moments[L].y, (float)block_spp[L >> 10], a.x, a.y, a.z);
	x0[p] = make_float4(d.x, d.y, d.z, d.w);
	x1[p] = make_float4(n.x, n.y, n.z, __float_as_int(g_hits[L].x) != -1 ? 1.0f : 0.0f);
	x2[p] = make_float4(q.x, q.y, q.z, (float)block_spp[L >> 10]); // (.w: the sample count, which only the temporal merge reads)
	xa[p] = make_float4(a.x, a.y, a.z, 0.0f);
}

struct DeviceImages {
	const float4 *a, *b, *c;
	__device__ __forceinline__ static Dn4 load(const float4 *p, int i) { const float4 v = p[i]; return Dn4{v.x, v.y, v.z, v.w}; }
	__device__ __forceinline__ Dn4 x0(int i) const { return load(a, i); }
	__device__ __forceinline__ Dn4 x1(int i) const { return load(b, i); }
	__device__ __forceinline__ Dn4 x2(int i) const { return load(c, i); }
};

constexpr int kAtrousX = 32, kAtrousY = 8; // a workgroup = 32 x 8 pixels: a wave reads two rows of 32 pixels x 16 bytes

// one pixel per thread; plain global loads (three 16-byte loads per tap): at these sizes the working set (48 B per pixel read) sits in the L2 / Infinity Cache
template <bool LAST>
__global__ __launch_bounds__(kAtrousX * kAtrousY) void k_atrous(const float4 *x0, const float4 *x1, const float4 *x2, const float4 *xa, float4 *x0_out, float *rgb, int width, int height,
                                                                 int step, float sigma_l, float sigma_z)
{
	const int x = blockIdx.x * kAtrousX + threadIdx.x, y = blockIdx.y * kAtrousY + threadIdx.y;
	if(x >= width || y >= height) return;
	const DeviceImages img{x0, x1, x2};
	const Dn4 r = denoise_level(img, width, height, x, y, step, sigma_l, sigma_z);
	const size_t p = (size_t)y * width + x;
	if(LAST)
	{
		float out[3];
		denoise_remodulate(r, DeviceImages::load(xa, (int)p), out);
		rgb[p * 3] = out[0]; rgb[p * 3 + 1] = out[1]; rgb[p * 3 + 2] = out[2];
	}
	else x0_out[p] = make_float4(r.x, r.y, r.z, r.w);
}

struct DeviceHistory {
	const float4 *a, *b, *c, *d;
	__device__ __forceinline__ Dn4 h0(int i) const { return DeviceImages::load(a, i); }
	__device__ __forceinline__ Dn4 h1(int i) const { return DeviceImages::load(b, i); }
	__device__ __forceinline__ Dn4 h2(int i) const { return DeviceImages::load(c, i); }
	__device__ __forceinline__ Dn4 ha(int i) const { return DeviceImages::load(d, i); }
};

// One pixel per thread, the workgroup of k_atrous.  Reads 64 B of the call's images and up to four taps x 64 B of the history (neighbouring pixels share
// them: 64 B per pixel reach the memory where the motion is smooth), writes the merged X0 (16 B), X2 with n_out in .w (16 B) and the history length
// (4 B): 164 B per pixel.  The history's camera comes by value.  MOTION: through k_motion_gather's XP, XN (32 B per pixel more), which the other
// instance never looks at (they stand last, so that its kernel arguments lie where they lay before there was a motion call).
template <bool MOTION>
__global__ __launch_bounds__(kAtrousX * kAtrousY) void k_temporal_merge(const float4 *x0, const float4 *x1, float4 *x2, const float4 *xa, const float4 *h0, const float4 *h1,
                                                                         const float4 *h2, const float4 *ha, float4 *merged, float *length, int width, int height, int have,
                                                                         TemporalCamera cam, float history_cap, const float4 *xp, const float4 *xn)
{
	const int x = blockIdx.x * kAtrousX + threadIdx.x, y = blockIdx.y * kAtrousY + threadIdx.y;
	if(x >= width || y >= height) return;
	const int p = y * width + x;
	const Dn4 c2 = DeviceImages::load(x2, p);
	const DeviceHistory hist{h0, h1, h2, ha};
	const TemporalOut r = MOTION ? temporal_merge_motion(hist, have != 0, cam, width, height, DeviceImages::load(x0, p), DeviceImages::load(x1, p), DeviceImages::load(xa, p), c2.w, history_cap,
	                                                     DeviceImages::load(xp, p), DeviceImages::load(xn, p))
	                             : temporal_merge(hist, have != 0, cam, width, height, DeviceImages::load(x0, p), DeviceImages::load(x1, p), c2, DeviceImages::load(xa, p), c2.w, history_cap);
	merged[p] = make_float4(r.x0.x, r.x0.y, r.x0.z, r.x0.w);
	x2[p] = make_float4(c2.x, c2.y, c2.z, r.n);
	length[p] = r.n;
}

constexpr int kSnapshotVecs = 5; // the first 80 bytes of a record: words 0..17, and the material id and the class word, which nothing here reads
static_assert(kSnapshotVecs * 4 >= kTemporalTriWords, "the snapshot holds the words temporal_previous_point reads");

// the snapshot: an array of 80-byte elements, so that the gather's five loads of one triangle lie in one or two cache lines.  One thread per float4: a
// workgroup copies kSnapshotGroup triangles, thread j the float4 j % 5 of its triangle j / 5 — 32-bit arithmetic, neighbouring lanes write neighbouring
// addresses.  It reads 80 of every record's 128 bytes: 1.3 x the traffic of a plain copy of what it writes
constexpr int kSnapshotGroup = 64;
__global__ __launch_bounds__(kSnapshotGroup * kSnapshotVecs) void k_motion_snapshot(const float4 *__restrict__ records, int tri_float4, int64_t n_tris, float4 *__restrict__ snapshot)
{
	const uint32_t j = threadIdx.x, t = j / kSnapshotVecs, k = j - t * kSnapshotVecs;
	const int64_t tri = (int64_t)blockIdx.x * kSnapshotGroup + t;
	if(tri >= n_tris) return;
	snapshot[(size_t)tri * kSnapshotVecs + k] = records[(size_t)tri * (size_t)tri_float4 + k];
}

__device__ __forceinline__ void unpack_tri(const float4 *__restrict__ q, float w[kSnapshotVecs * 4])
{
#pragma unroll
	for(int k = 0; k < kSnapshotVecs; ++k)
	{
		const float4 v = q[k];
		w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
	}
}

// One thread per local pixel of the block list, as k_denoise_prepare.  Reads the hit (16 B) and the normal and position guides (32 B), and where the hit
// triangle's index lies inside the snapshot (n_known triangles: 0 when there is none) 80 B of the snapshot and 80 B of the record — a gather by triangle
// index, coherent only between neighbouring pixels; writes XP and XN (32 B).  An index outside [0, n_known) is never used as one.  Every array of a
// lane is indexed by constants after unrolling: registers, no scratch.
__global__ __launch_bounds__(256) void k_motion_gather(const float4 *__restrict__ g_hits, const float4 *__restrict__ g_normal, const float4 *__restrict__ g_position,
                                                       const int32_t *__restrict__ blocks, int n_px, int blocks_x, int width, int height, const float4 *__restrict__ snapshot,
                                                       int64_t n_known, const float4 *__restrict__ records, int tri_float4, float4 *__restrict__ xp, float4 *__restrict__ xn)
{
	const int L = blockIdx.x * blockDim.x + threadIdx.x;
	if(L >= n_px) return;
	int x, y;
	block_pixel_xy(blocks[L >> 10], L & 1023, blocks_x, &x, &y);
	if(x >= width || y >= height) return;
	const size_t p = (size_t)y * width + x;
	const float4 hq = g_hits[L], n = g_normal[L], q = g_position[L];
	const int32_t tri = __float_as_int(hq.x);
	const bool known = tri >= 0 && (int64_t)tri < n_known;
	float prev[kSnapshotVecs * 4] = {}, cur[kSnapshotVecs * 4] = {};
	if(known)
	{
		unpack_tri(snapshot + (size_t)tri * kSnapshotVecs, prev);
		unpack_tri(records + (size_t)tri * (size_t)tri_float4, cur);
	}
	const TemporalPrevious r = temporal_previous_point(prev, cur, known, hq.y, hq.z, Dn4{n.x, n.y, n.z, tri != -1 ? 1.0f : 0.0f}, Dn4{q.x, q.y, q.z, 0.0f});
	xp[p] = make_float4(r.xp.x, r.xp.y, r.xp.z, r.xp.w);
	xn[p] = make_float4(r.xn.x, r.xn.y, r.xn.z, r.xn.w);
}

// the block-major images of a set of blocks on one device: a context's own (accum and moments are then the context's) or the merged ones of all devices
struct LocalImages {
	const float4 *accum; const float2 *moments; const int32_t *blocks, *block_spp;
	const float4 *albedo, *normal, *position, *hits;
	int n_blocks;
};

constexpr int kTimingEvents = 4 + kDenoiseMaxLevels; // start, guides, prepare, (the temporal merge,) every level

// what adypt_denoise_temporal adds to a call
struct TemporalCall { float history_cap; bool commit; bool motion; }; // motion: adypt_denoise_temporal_motion

// Everything the denoiser keeps per context; parked in the context (ctx_attachment), freed by adypt_destroy (the context's device is current then).
struct Denoiser {
	int width = 0, height = 0;
	// guide scratch of the owned blocks, block-major: 64 B per local pixel + 4 B per owned block
	Buffer<float4> g_albedo, g_normal, g_position, g_hits;
	Buffer<int32_t> d_block_spp;
	// the filter's row-major images of the whole picture: 80 B + 12 B (the result) per image pixel
	Buffer<float4> x0[2], x1, x2, xa;
	Buffer<float> rgb;
	// several devices: the block-major images of every device's blocks, back to back in rank order, on the first device (88 B per pixel of the blocks
	// + 8 B per block)
	Buffer<float4> m_accum, m_albedo, m_normal, m_position, m_hits;
	Buffer<float2> m_moments;
	Buffer<int32_t> m_blocks, m_block_spp;
	// the temporal merge, allocated at the first temporal call only: the merged image of the call, the history (what the last committing call left:
	// its merged image, its X1, X2 with n_out in .w, XA — swapped in, never copied — and its camera) and the length read-out: 84 B per image pixel
	Buffer<float4> xm, h0, h1, h2, ha;
	Buffer<float> length;
	TemporalCamera h_camera;
	bool have_history = false, have_length = false;
	StageTimer<kTimingEvents> timer; // completed: the last filter ran to its end, rgb is its result
	int levels_timed = 0;
	bool merge_timed = false; // the last filter was a temporal call: the merge's stage stands between prepare's and the first level's
	// following moved geometry.  XP, XN: 32 B per image pixel, allocated at the first motion call.  The snapshot belongs to the history: 80 B per
	// triangle, allocated at the first committing motion call, written only on such a commit, dropped with the history, by a committing temporal call
	// without motion (the history's geometry is then unknown) and by adypt_set_triangles (the indices mean other triangles)
	Buffer<float4> xp, xn, snapshot;
	int64_t snapshot_tris = 0;
	bool have_snapshot = false, have_motion = false;
	StageTimer<2> snapshot_timer; // the copy kernel of the last commit
	void drop_snapshot() { have_snapshot = false; snapshot_tris = 0; }
};

Denoiser *denoiser_of(adypt_ctx *c) { return ctx_state<Denoiser>(c, kAttachDenoise); }
Denoiser *finished_denoiser(adypt_ctx *c) { Denoiser *d = ctx_state_if_any<Denoiser>(c, kAttachDenoise); return d && d->timer.completed() ? d : nullptr; }

// the guide scratch of the context's own blocks (allocated at the first call: the size never changes)
int ensure_guides(adypt_ctx *c, Denoiser *d, const CtxInfo &i)
{
	const size_t n = (size_t)std::max(i.n_local_px, 64);
	CTX_TRY(c, at_least(d->g_albedo, n)); CTX_TRY(c, at_least(d->g_normal, n)); CTX_TRY(c, at_least(d->g_position, n)); CTX_TRY(c, at_least(d->g_hits, n));
	CTX_TRY(c, at_least(d->d_block_spp, (size_t)std::max(i.n_local_px / kBlockPixels, 1)));
	return ADYPT_OK;
}

int ensure_filter_images(adypt_ctx *c, Denoiser *d, const CtxInfo &i)
{
	const size_t n = (size_t)i.width * (size_t)i.height;
	d->width = i.width; d->height = i.height;
	CTX_TRY(c, at_least(d->x0[0], n)); CTX_TRY(c, at_least(d->x0[1], n)); CTX_TRY(c, at_least(d->x1, n)); CTX_TRY(c, at_least(d->x2, n)); CTX_TRY(c, at_least(d->xa, n));
	CTX_TRY(c, at_least(d->rgb, n * 3));
	return ADYPT_OK;
}

int ensure_history_images(adypt_ctx *c, Denoiser *d)
{
	const size_t n = (size_t)d->width * (size_t)d->height;
	CTX_TRY(c, at_least(d->xm, n)); CTX_TRY(c, at_least(d->h0, n)); CTX_TRY(c, at_least(d->h1, n)); CTX_TRY(c, at_least(d->h2, n)); CTX_TRY(c, at_least(d->ha, n));
	CTX_TRY(c, at_least(d->length, n));
	return ADYPT_OK;
}

// The snapshot of a committing motion call: the records as they are now, enqueued on `stream` behind the call's gather, which reads the old one.  The
// history has none until the caller has waited for the stream and keeps it (keep_snapshot): a failure in between leaves every pixel unmoved.
int enqueue_snapshot(adypt_ctx *c, Denoiser *d, hipStream_t stream)
{
	const CtxScene sc = ctx_scene(c);
	const int64_t n_vecs = sc.n_tris * kSnapshotVecs;
	d->drop_snapshot(); // (a failure below leaves none: every pixel is then unmoved)
	d->snapshot_timer.invalidate();
	CTX_TRY(c, at_least(d->snapshot, (size_t)n_vecs));
	CTX_TRY(c, d->snapshot_timer.mark(0, stream));
	hipLaunchKernelGGL(k_motion_snapshot, dim3(grid_of(sc.n_tris, kSnapshotGroup)), dim3(kSnapshotGroup * kSnapshotVecs), 0, stream, (const float4 *)sc.triangles, sc.tri_float4, sc.n_tris,
	                   d->snapshot.get());
	CTX_TRY(c, hipGetLastError());
	CTX_TRY(c, d->snapshot_timer.mark(1, stream));
	return ADYPT_OK;
}
void keep_snapshot(adypt_ctx *c, Denoiser *d)
{
	d->snapshot_timer.complete();
	d->snapshot_tris = ctx_scene(c).n_tris;
	d->have_snapshot = true;
}

// prepare (+ the temporal merge) + the levels, on `stream`; d's images are the whole picture's (ensure_filter_images).  t: a temporal call, under the
// camera `cam` of the context the guides were captured by.
int run_filter(adypt_ctx *c, Denoiser *d, hipStream_t stream, const LocalImages &in, const DenoiseParams &prm, const TemporalCall *t = nullptr, const CtxCamera *cam = nullptr)
{
	if(t) CTX_STEP(ensure_history_images(c, d));
	const bool motion = t && t->motion;
	if(motion)
	{
		const size_t n = (size_t)d->width * (size_t)d->height;
		CTX_TRY(c, at_least(d->xp, n)); CTX_TRY(c, at_least(d->xn, n));
		d->have_motion = false;
	}
	const int width = d->width, height = d->height, n_px = in.n_blocks * kBlockPixels;
	const int blocks_x = (width + kBlockDim - 1) / kBlockDim;
	hipLaunchKernelGGL(k_denoise_prepare, dim3(grid_of(n_px, 256)), dim3(256), 0, stream, in.accum, in.moments, in.blocks, in.block_spp, n_px, blocks_x, width, height, in.albedo,
	                   in.normal, in.position, in.hits, d->x0[0].get(), d->x1.get(), d->x2.get(), d->xa.get());
	CTX_TRY(c, hipGetLastError());
	CTX_TRY(c, d->timer.mark(2, stream));
	const dim3 grid(grid_of(width, kAtrousX), grid_of(height, kAtrousY)), block(kAtrousX, kAtrousY);
	const int first = t ? 4 : 3; // the mark behind level 0
	if(t)
	{
		d->have_length = false;
		if(motion)
		{
			// (a snapshot of another triangle count is none: adypt_set_triangles drops it, so this only guards)
			const CtxScene sc = ctx_scene(c);
			const int64_t n_known = d->have_history && d->have_snapshot && d->snapshot_tris == sc.n_tris ? d->snapshot_tris : 0;
			hipLaunchKernelGGL(k_motion_gather, dim3(grid_of(n_px, 256)), dim3(256), 0, stream, in.hits, in.normal, in.position, in.blocks, n_px, blocks_x, width, height,
			                   (const float4 *)d->snapshot, n_known, (const float4 *)sc.triangles, sc.tri_float4, d->xp.get(), d->xn.get());
			CTX_TRY(c, hipGetLastError());
		}
		const auto merge = motion ? k_temporal_merge<true> : k_temporal_merge<false>;
		hipLaunchKernelGGL(merge, grid, block, 0, stream, (const float4 *)d->x0[0], (const float4 *)d->x1, d->x2.get(), (const float4 *)d->xa, (const float4 *)d->h0,
		                   (const float4 *)d->h1, (const float4 *)d->h2, (const float4 *)d->ha, d->xm.get(), d->length.get(), width, height, d->have_history ? 1 : 0, d->h_camera,
		                   t->history_cap, (const float4 *)d->xp, (const float4 *)d->xn);
		CTX_TRY(c, hipGetLastError());
		CTX_TRY(c, d->timer.mark(3, stream));
	}
	for(int l = 0; l < prm.levels; ++l)
	{
		const float4 *src = (l == 0 && t) ? d->xm : d->x0[l & 1];
		float4 *dst = d->x0[(l & 1) ^ 1];
		if(l == prm.levels - 1)
			hipLaunchKernelGGL(k_atrous<true>, grid, block, 0, stream, src, (const float4 *)d->x1, (const float4 *)d->x2, (const float4 *)d->xa, dst, d->rgb.get(), width, height, 1 << l, prm.sigma_l, prm.sigma_z);
		else
			hipLaunchKernelGGL(k_atrous<false>, grid, block, 0, stream, src, (const float4 *)d->x1, (const float4 *)d->x2, (const float4 *)d->xa, dst, d->rgb.get(), width, height, 1 << l, prm.sigma_l, prm.sigma_z);
		CTX_TRY(c, hipGetLastError());
		CTX_TRY(c, d->timer.mark(first + l, stream));
	}
	d->levels_timed = prm.levels;
	d->merge_timed = t != nullptr;
	if(motion && t->commit) CTX_STEP(enqueue_snapshot(c, d, stream));
	CTX_TRY(c, hipStreamSynchronize(stream));
	d->timer.complete();
	if(t)
	{
		d->have_length = true;
		if(motion) d->have_motion = true;
		if(t->commit)
		{
			// the snapshot goes with the history: the records of this call, or none
			if(motion) keep_snapshot(c, d);
			else d->drop_snapshot();
			// this call's merged image, guides (X2.w = n_out) and camera become the history; what the history held is overwritten by the next prepare
			std::swap(d->xm, d->h0); std::swap(d->x1, d->h1); std::swap(d->x2, d->h2); std::swap(d->xa, d->ha);
			d->h_camera = temporal_camera(cam->origin, cam->inv_proj, cam->inv_view);
			d->have_history = true;
		}
	}
	return ADYPT_OK;
}

int params_of(const adypt_denoise_params *p, DenoiseParams *out, std::string *why, const char *fn)
{
	*out = p ? DenoiseParams{p->levels, p->sigma_l, p->sigma_z} : kDenoiseDefaults;
	if(denoise_params_valid(*out)) return ADYPT_OK;
	*why = std::string(fn) + ": levels must be in [1, " + std::to_string(kDenoiseMaxLevels) + "], sigma_l and sigma_z positive numbers";
	return ADYPT_E_INVALID;
}

// the context's guides into its own scratch, enqueued behind its frames
int capture_guides(adypt_ctx *c, Denoiser *d, const CtxInfo &i, const char *fn)
{
	CTX_STEP(ensure_guides(c, d, i));
	return ctx_capture_guides(c, fn, d->g_albedo, d->g_normal, d->g_position, d->g_hits);
}

int read_result(adypt_ctx *c, const char *fn, float *rgb)
{
	Denoiser *d = finished_denoiser(c);
	if(!d) return ctx_fail(c, ADYPT_E_STATE, std::string(fn) + ": nothing has been denoised yet (adypt_denoise)");
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_TRY(c, hipMemcpyAsync(rgb, d->rgb, (size_t)d->width * d->height * 3 * sizeof(float), hipMemcpyDeviceToHost, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	return ADYPT_OK;
}

// one block-major local image of a context (n_local_px > 0 elements) on the host (the stream is drained when it returns)
template <class T> int fetch(adypt_ctx *c, const CtxInfo &i, const T *device, T *host)
{
	CTX_TRY(c, hipMemcpyAsync(host, device, (size_t)i.n_local_px * sizeof(T), hipMemcpyDeviceToHost, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	return ADYPT_OK;
}

// the temporal half of a call's parameters (tp NULL = the defaults: cap 64, committing)
int temporal_of(const adypt_temporal_params *tp, bool motion, TemporalCall *out, std::string *why, const char *fn)
{
	*out = tp ? TemporalCall{tp->history_cap, tp->commit != 0, motion} : TemporalCall{kTemporalDefaultCap, true, motion};
	if(temporal_cap_valid(out->history_cap)) return ADYPT_OK;
	*why = std::string(fn) + ": history_cap must be a positive finite number";
	return ADYPT_E_INVALID;
}

// adypt_denoise (temporal false: tp is not looked at), adypt_denoise_temporal and (motion) adypt_denoise_temporal_motion of one context
int denoise_context(adypt_ctx *c, const adypt_denoise_params *p, const adypt_temporal_params *tp, bool temporal, const char *fn, bool motion = false)
{
	if(!c) return ADYPT_E_INVALID;
	DenoiseParams prm;
	TemporalCall t;
	std::string why;
	if(params_of(p, &prm, &why, fn) != ADYPT_OK) return ctx_fail(c, ADYPT_E_INVALID, why);
	if(temporal && temporal_of(tp, motion, &t, &why, fn) != ADYPT_OK) return ctx_fail(c, ADYPT_E_INVALID, why);
	const CtxInfo i = ctx_info(c);
	if(i.nranks != 1) return ctx_fail(c, ADYPT_E_STATE, std::string(fn) + ": the context is a tile shard (tile_nranks > 1): the filter needs the whole image (adypt_multi_denoise)");
	CTX_STEP(ctx_denoise_ready(c, fn));
	CTX_TRY(c, hipSetDevice(i.device));
	Denoiser *d = denoiser_of(c);
	CTX_STEP(ensure_filter_images(c, d, i));
	d->timer.invalidate();
	CTX_TRY(c, d->timer.mark(0, i.stream));
	CTX_STEP(capture_guides(c, d, i, fn));
	CTX_TRY(c, d->timer.mark(1, i.stream));
	const DenoiseInputs in = ctx_denoise_inputs(c);
	CTX_TRY(c, hipMemcpyAsync(d->d_block_spp, in.block_spp.data(), in.block_spp.size() * sizeof(int32_t), hipMemcpyHostToDevice, i.stream));
	const LocalImages local{in.accum, in.moments, in.blocks, d->d_block_spp, d->g_albedo, d->g_normal, d->g_position, d->g_hits, in.n_blocks};
	const CtxCamera cam = ctx_camera(c);
	return run_filter(c, d, i.stream, local, prm, temporal ? &t : nullptr, &cam);
}

int read_history_length(adypt_ctx *c, const char *fn, float *length)
{
	Denoiser *d = finished_denoiser(c);
	if(!d || !d->have_length) return ctx_fail(c, ADYPT_E_STATE, std::string(fn) + ": no temporal call has run yet (adypt_denoise_temporal)");
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	CTX_TRY(c, hipMemcpyAsync(length, d->length, (size_t)d->width * d->height * sizeof(float), hipMemcpyDeviceToHost, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	return ADYPT_OK;
}

// XP, XN of the last motion call: the previous position (W x H x 3 floats) and the moved flag (W x H bytes) of every pixel; either may be null
int read_motion(adypt_ctx *c, const char *fn, float *prev_position, uint8_t *moved)
{
	Denoiser *d = finished_denoiser(c);
	if(!d || !d->have_motion) return ctx_fail(c, ADYPT_E_STATE, std::string(fn) + ": no motion call has run yet (adypt_denoise_temporal_motion)");
	const CtxInfo i = ctx_info(c);
	CTX_TRY(c, hipSetDevice(i.device));
	const size_t n = (size_t)d->width * d->height;
	std::vector<float4> xp(n);
	CTX_TRY(c, hipMemcpyAsync(xp.data(), d->xp, n * sizeof(float4), hipMemcpyDeviceToHost, i.stream));
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	for(size_t k = 0; k < n; ++k)
	{
		if(prev_position) { prev_position[3 * k] = xp[k].x; prev_position[3 * k + 1] = xp[k].y; prev_position[3 * k + 2] = xp[k].z; }
		if(moved) moved[k] = xp[k].w != 0.0f ? 1 : 0;
	}
	return ADYPT_OK;
}

int get_motion(adypt_ctx *c, const char *fn, adypt_denoise_motion *out)
{
	if(!out) return ctx_fail(c, ADYPT_E_INVALID, std::string(fn) + ": out is null");
	*out = adypt_denoise_motion{};
	const Denoiser *d = ctx_state_if_any<Denoiser>(c, kAttachDenoise);
	if(!d) return ADYPT_OK;
	out->have_snapshot = d->have_snapshot ? 1 : 0;
	out->n_tris = d->snapshot_tris;
	out->device_bytes = (int64_t)(d->snapshot.bytes() + d->xp.bytes() + d->xn.bytes());
	if(d->have_snapshot) (void)d->snapshot_timer.read(&out->snapshot_ms, 1, 1, false);
	return ADYPT_OK;
}

int read_merge_ms(adypt_ctx *c, const char *fn, float *ms)
{
	Denoiser *d = finished_denoiser(c);
	if(!d || !d->merge_timed) return ctx_fail(c, ADYPT_E_STATE, std::string(fn) + ": the last filter was not a temporal call (adypt_denoise_temporal)");
	float all[kTimingEvents];
	d->timer.read(all, kTimingEvents, 3 + d->levels_timed, false);
	*ms = all[2];
	return ADYPT_OK;
}

}  // namespace

namespace adypt {

void denoise_drop_snapshot(adypt_ctx *c)
{
	Denoiser *d = ctx_state_if_any<Denoiser>(c, kAttachDenoise);
	if(!d) return;
	d->drop_snapshot();
	d->snapshot.release();
}

}  // namespace adypt

extern "C" {

int adypt_denoise(adypt_ctx *c, const adypt_denoise_params *p) { return denoise_context(c, p, nullptr, false, "adypt_denoise"); }

int adypt_denoise_temporal(adypt_ctx *c, const adypt_denoise_params *p, const adypt_temporal_params *tp) { return denoise_context(c, p, tp, true, "adypt_denoise_temporal"); }

int adypt_denoise_temporal_motion(adypt_ctx *c, const adypt_denoise_params *p, const adypt_temporal_params *tp)
{
	return denoise_context(c, p, tp, true, "adypt_denoise_temporal_motion", true);
}

int adypt_denoise_history_reset(adypt_ctx *c)
{
	if(!c) return ADYPT_E_INVALID;
	if(Denoiser *d = ctx_state_if_any<Denoiser>(c, kAttachDenoise)) { d->have_history = false; d->drop_snapshot(); }
	return ADYPT_OK;
}

int adypt_read_denoise_motion(adypt_ctx *c, float *prev_position, uint8_t *moved)
{
	if(!c) return ADYPT_E_INVALID;
	return read_motion(c, "adypt_read_denoise_motion", prev_position, moved);
}

int adypt_get_denoise_motion(adypt_ctx *c, adypt_denoise_motion *out)
{
	if(!c) return ADYPT_E_INVALID;
	return get_motion(c, "adypt_get_denoise_motion", out);
}

int adypt_read_denoise_history(adypt_ctx *c, float *length)
{
	if(!c || !length) return ADYPT_E_INVALID;
	return read_history_length(c, "adypt_read_denoise_history", length);
}

int adypt_get_denoise_merge_ms(adypt_ctx *c, float *ms)
{
	if(!c || !ms) return ADYPT_E_INVALID;
	return read_merge_ms(c, "adypt_get_denoise_merge_ms", ms);
}

int adypt_read_denoised(adypt_ctx *c, float *rgb)
{
	if(!c || !rgb) return ADYPT_E_INVALID;
	return read_result(c, "adypt_read_denoised", rgb);
}

int adypt_read_denoise_guides(adypt_ctx *c, float *albedo, float *normal, float *position, uint8_t *hit)
{
	if(!c) return ADYPT_E_INVALID;
	const CtxInfo i = ctx_info(c);
	if(i.n_local_px == 0) return ADYPT_OK; // a shard that owns no block
	CTX_TRY(c, hipSetDevice(i.device));
	Denoiser *d = denoiser_of(c);
	CTX_STEP(capture_guides(c, d, i, "adypt_read_denoise_guides"));
	const std::vector<int32_t> blocks = owned_blocks(i.width, i.height, i.rank, i.nranks);
	std::vector<float4> local((size_t)i.n_local_px);
	float *const image[3] = {albedo, normal, position};
	const float4 *const device[3] = {d->g_albedo, d->g_normal, d->g_position};
	for(int k = 0; k < 3; ++k)
	{
		if(!image[k]) continue;
		CTX_STEP(fetch(c, i, device[k], local.data()));
		for_each_local_pixel(blocks, i.width, i.height, [&](size_t L, int x, int y) {
			float *o = image[k] + ((size_t)y * i.width + x) * 3;
			o[0] = local[L].x; o[1] = local[L].y; o[2] = local[L].z;
		});
	}
	if(hit)
	{
		CTX_STEP(fetch(c, i, (const float4 *)d->g_hits, local.data()));
		for_each_local_pixel(blocks, i.width, i.height, [&](size_t L, int x, int y) {
			int32_t tri;
			memcpy(&tri, &local[L].x, 4);
			hit[(size_t)y * i.width + x] = tri != -1 ? 1 : 0;
		});
	}
	CTX_TRY(c, hipStreamSynchronize(i.stream));
	return ADYPT_OK;
}

int adypt_get_denoise_timing(adypt_ctx *c, float *ms, int capacity)
{
	if(!c || !ms || capacity < 0) return ADYPT_E_INVALID;
	Denoiser *d = finished_denoiser(c);
	if(!d) return ctx_fail(c, ADYPT_E_STATE, "adypt_get_denoise_timing: nothing has been denoised yet (adypt_denoise)");
	const int n = 2 + d->levels_timed;
	if(!d->merge_timed) return d->timer.read(ms, capacity, n, false);
	// a temporal call: the merge's stage (adypt_get_denoise_merge_ms) is left out, the layout is adypt_denoise's
	if(capacity < n) return n;
	float all[kTimingEvents];
	d->timer.read(all, kTimingEvents, n + 1, false);
	for(int k = 0; k < n; ++k) ms[k] = all[k < 2 ? k : k + 1];
	return n;
}

// ---- one process, N devices ----
}  // extern "C"

namespace {

// adypt_multi_denoise and adypt_multi_denoise_temporal: the merge runs on the first device, where the filter runs, and the history lives there
int multi_denoise(adypt_multi *m, const adypt_denoise_params *p, const adypt_temporal_params *tp, bool temporal, const char *fn, bool motion = false)
{
	const int n_dev = adypt_multi_device_count(m);
	if(n_dev < 1) return ADYPT_E_INVALID;
	adypt_ctx *root = adypt_multi_context(m, 0);
	if(n_dev == 1) return multi_each(m, [=](adypt_ctx *c) { return denoise_context(c, p, tp, temporal, fn, motion); });
	auto fail_ctx = [m](adypt_ctx *c, int r) { multi_set_error(m, adypt_last_error(c)); return r; };
	DenoiseParams prm;
	TemporalCall t;
	std::string why;
	if(params_of(p, &prm, &why, fn) != ADYPT_OK) { multi_set_error(m, why); return ADYPT_E_INVALID; }
	if(temporal && temporal_of(tp, motion, &t, &why, fn) != ADYPT_OK) { multi_set_error(m, why); return ADYPT_E_INVALID; }
	std::vector<adypt_ctx *> ctx;
	for(int k = 0; k < n_dev; ++k) ctx.push_back(adypt_multi_context(m, k));
	CTX_STEP(multi_each(m, [fn](adypt_ctx *c) { return ctx_denoise_ready(c, fn); }));
	// every device captures the guides of its own blocks: all enqueued before the first is waited for
	CTX_STEP(multi_each(m, [fn](adypt_ctx *c) {
		const CtxInfo i = ctx_info(c);
		if(i.n_local_px == 0) return (int)ADYPT_OK;
		if(hipSetDevice(i.device) != hipSuccess) return ctx_fail(c, ADYPT_E_HIP, std::string(fn) + ": hipSetDevice failed");
		return capture_guides(c, denoiser_of(c), i, fn);
	}));
	// the local images of every device back to back in rank order, and their block lists and sample counts likewise (the counts from each context's
	// own state in that order: multi.hip's merge is sorted by block index, which is not this order, and would launch k_noise_blocks for nothing)
	const CtxInfo ri = ctx_info(root);
	size_t n_px = 0;
	for(adypt_ctx *c : ctx) n_px += (size_t)ctx_info(c).n_local_px;
	const int n_blocks = (int)(n_px / kBlockPixels);
	std::vector<float4> accum(n_px), albedo(n_px), normal(n_px), position(n_px), hits(n_px);
	std::vector<float2> moments(n_px);
	std::vector<int32_t> blocks, block_spp;
	size_t at = 0; // the rank's first pixel in them
	for(adypt_ctx *c : ctx)
	{
		const CtxInfo i = ctx_info(c);
		if(i.n_local_px == 0) continue;
		if(hipSetDevice(i.device) != hipSuccess) return fail_ctx(c, ctx_fail(c, ADYPT_E_HIP, std::string(fn) + ": hipSetDevice failed"));
		Denoiser *d = denoiser_of(c);
		const DenoiseInputs in = ctx_denoise_inputs(c);
		const float4 *const device[5] = {in.accum, d->g_albedo, d->g_normal, d->g_position, d->g_hits};
		float4 *const merged[5] = {accum.data(), albedo.data(), normal.data(), position.data(), hits.data()};
		int r = fetch(c, i, in.moments, moments.data() + at);
		for(int k = 0; k < 5 && r == ADYPT_OK; ++k) r = fetch(c, i, device[k], merged[k] + at);
		if(r != ADYPT_OK) return fail_ctx(c, r);
		blocks.insert(blocks.end(), in.block_index.begin(), in.block_index.end());
		block_spp.insert(block_spp.end(), in.block_spp.begin(), in.block_spp.end());
		at += (size_t)i.n_local_px;
	}
	// ... uploaded to the first device, where the same prepare / a-trous launches run
	adypt_ctx *c = root;
	auto steps = [&]() -> int {
		CTX_TRY(c, hipSetDevice(ri.device));
		Denoiser *d = denoiser_of(c);
		CTX_STEP(ensure_filter_images(c, d, ri));
		d->timer.invalidate();
		CTX_TRY(c, at_least(d->m_accum, n_px)); CTX_TRY(c, at_least(d->m_albedo, n_px)); CTX_TRY(c, at_least(d->m_normal, n_px)); CTX_TRY(c, at_least(d->m_position, n_px));
		CTX_TRY(c, at_least(d->m_hits, n_px)); CTX_TRY(c, at_least(d->m_moments, n_px)); CTX_TRY(c, at_least(d->m_blocks, (size_t)n_blocks)); CTX_TRY(c, at_least(d->m_block_spp, (size_t)n_blocks));
		CTX_TRY(c, d->timer.mark(0, ri.stream));
		CTX_TRY(c, hipMemcpyAsync(d->m_accum, accum.data(), n_px * sizeof(float4), hipMemcpyHostToDevice, ri.stream));
		CTX_TRY(c, hipMemcpyAsync(d->m_albedo, albedo.data(), n_px * sizeof(float4), hipMemcpyHostToDevice, ri.stream));
		CTX_TRY(c, hipMemcpyAsync(d->m_normal, normal.data(), n_px * sizeof(float4), hipMemcpyHostToDevice, ri.stream));
		CTX_TRY(c, hipMemcpyAsync(d->m_position, position.data(), n_px * sizeof(float4), hipMemcpyHostToDevice, ri.stream));
		CTX_TRY(c, hipMemcpyAsync(d->m_hits, hits.data(), n_px * sizeof(float4), hipMemcpyHostToDevice, ri.stream));
		CTX_TRY(c, hipMemcpyAsync(d->m_moments, moments.data(), n_px * sizeof(float2), hipMemcpyHostToDevice, ri.stream));
		CTX_TRY(c, hipMemcpyAsync(d->m_blocks, blocks.data(), blocks.size() * sizeof(int32_t), hipMemcpyHostToDevice, ri.stream));
		CTX_TRY(c, hipMemcpyAsync(d->m_block_spp, block_spp.data(), block_spp.size() * sizeof(int32_t), hipMemcpyHostToDevice, ri.stream));
		CTX_TRY(c, d->timer.mark(1, ri.stream));
		const LocalImages all{d->m_accum, d->m_moments, d->m_blocks, d->m_block_spp, d->m_albedo, d->m_normal, d->m_position, d->m_hits, n_blocks};
		const CtxCamera cam = ctx_camera(c); // (adypt_multi_set_camera gives every context the same)
		return run_filter(c, d, ri.stream, all, prm, temporal ? &t : nullptr, &cam);
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

}  // namespace

extern "C" {

int adypt_multi_denoise(adypt_multi *m, const adypt_denoise_params *p) { return multi_denoise(m, p, nullptr, false, "adypt_multi_denoise"); }

int adypt_multi_denoise_temporal(adypt_multi *m, const adypt_denoise_params *p, const adypt_temporal_params *tp) { return multi_denoise(m, p, tp, true, "adypt_multi_denoise_temporal"); }

int adypt_multi_denoise_temporal_motion(adypt_multi *m, const adypt_denoise_params *p, const adypt_temporal_params *tp)
{
	return multi_denoise(m, p, tp, true, "adypt_multi_denoise_temporal_motion", true);
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
	if(!length) return ADYPT_E_INVALID;
	return on_root(m, [=](adypt_ctx *c) { return read_history_length(c, "adypt_multi_read_denoise_history", length); });
}

int adypt_multi_get_denoise_merge_ms(adypt_multi *m, float *ms)
{
	if(!ms) return ADYPT_E_INVALID;
	return on_root(m, [=](adypt_ctx *c) { return read_merge_ms(c, "adypt_multi_get_denoise_merge_ms", ms); });
}

int adypt_multi_read_denoised(adypt_multi *m, float *rgb)
{
	if(adypt_multi_device_count(m) < 1 || !rgb) return ADYPT_E_INVALID;
	adypt_ctx *root = adypt_multi_context(m, 0);
	const int r = read_result(root, "adypt_multi_read_denoised", rgb);
	if(r != ADYPT_OK) multi_set_error(m, adypt_last_error(root));
	return r;
}

// every device writes the pixels of its own tiles
int adypt_multi_read_denoise_guides(adypt_multi *m, float *albedo, float *normal, float *position, uint8_t *hit)
{
	return multi_each(m, [=](adypt_ctx *c) { return adypt_read_denoise_guides(c, albedo, normal, position, hit); });
}

}  // extern "C"
