// The denoiser's kernels and the shape each is launched with, in a header of their own so that two libraries compile the same text: denoise.hip, which
// is the product, and csrc/probe/probe.hip, which runs every kernel on arrays a test makes (tests/test_gpu_denoise_probes.py).  The kernels stay in the
// anonymous namespace: each including unit has its own copies, and nothing here is visible outside it.  Who launches a kernel takes the grid and the
// workgroup from the *_launch function beside it — denoise.hip and the probe alike — so that the probe's launch shape cannot drift from the product's.
// What the stages are and in which order they run: the head of denoise.hip.
#pragma once
#include "tile_layout.hpp"
#include "denoise.hpp"
#include "temporal.hpp"

#include <hip/hip_runtime.h>

namespace {

using namespace adypt;

struct LaunchShape { dim3 grid, block; };

constexpr int kPixelThreads = 256; // the workgroup of the kernels that run one thread per local pixel of a block list: prepare and gather

// one thread per local pixel of a block list of n_px local pixels
inline LaunchShape local_pixels_launch(int n_px) { return LaunchShape{dim3((unsigned)(((int64_t)n_px + kPixelThreads - 1) / kPixelThreads)), dim3(kPixelThreads)}; }

__global__ __launch_bounds__(kPixelThreads) void k_denoise_prepare(const float4 *accum, const float2 *moments, const int32_t *blocks, const int32_t *block_spp, int n_px, int blocks_x, int width,
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
inline LaunchShape prepare_launch(int n_px) { return local_pixels_launch(n_px); }

struct DeviceImages {
	const float4 *a, *b, *c;
	__device__ __forceinline__ static Dn4 load(const float4 *p, int i) { const float4 v = p[i]; return Dn4{v.x, v.y, v.z, v.w}; }
	__device__ __forceinline__ Dn4 x0(int i) const { return load(a, i); }
	__device__ __forceinline__ Dn4 x1(int i) const { return load(b, i); }
	__device__ __forceinline__ Dn4 x2(int i) const { return load(c, i); }
};

constexpr int kAtrousX = 32, kAtrousY = 8; // a workgroup = 32 x 8 pixels: a wave reads two rows of 32 pixels x 16 bytes

// one thread per pixel of the width x height picture in workgroups of kAtrousX x kAtrousY: the levels, the merge and the window statistics
inline LaunchShape image_launch(int width, int height)
{
	return LaunchShape{dim3((unsigned)((width + kAtrousX - 1) / kAtrousX), (unsigned)((height + kAtrousY - 1) / kAtrousY)), dim3(kAtrousX, kAtrousY)};
}

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
inline LaunchShape atrous_launch(int width, int height) { return image_launch(width, height); }

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
// instance never looks at (they stand last, so that its kernel arguments lie where they lay before there was a motion call).  RECTIFY: the history is held
// against k_rectify_window's R0, R1 (32 B per pixel more read) and the share of its length it kept is written (4 B); these stand last in turn, and the
// instances without it pass temporal_merge a constant "off": their code is what it was.
template <bool MOTION, bool RECTIFY>
__global__ __launch_bounds__(kAtrousX * kAtrousY) void k_temporal_merge(const float4 *x0, const float4 *x1, float4 *x2, const float4 *xa, const float4 *h0, const float4 *h1,
                                                                         const float4 *h2, const float4 *ha, float4 *merged, float *length, int width, int height, int have,
                                                                         TemporalCamera cam, float history_cap, const float4 *xp, const float4 *xn, const float4 *r0, const float4 *r1, float *kept,
                                                                         float gamma)
{
	const int x = blockIdx.x * kAtrousX + threadIdx.x, y = blockIdx.y * kAtrousY + threadIdx.y;
	if(x >= width || y >= height) return;
	const int p = y * width + x;
	const Dn4 c2 = DeviceImages::load(x2, p);
	const DeviceHistory hist{h0, h1, h2, ha};
	Rectify rect;
	if(RECTIFY) rect = Rectify{true, DeviceImages::load(r0, p), DeviceImages::load(r1, p), gamma};
	const TemporalOut r = MOTION ? temporal_merge_motion(hist, have != 0, cam, width, height, DeviceImages::load(x0, p), DeviceImages::load(x1, p), DeviceImages::load(xa, p), c2.w, history_cap,
	                                                     DeviceImages::load(xp, p), DeviceImages::load(xn, p), rect)
	                             : temporal_merge(hist, have != 0, cam, width, height, DeviceImages::load(x0, p), DeviceImages::load(x1, p), c2, DeviceImages::load(xa, p), c2.w, history_cap, rect);
	merged[p] = make_float4(r.x0.x, r.x0.y, r.x0.z, r.x0.w);
	x2[p] = make_float4(c2.x, c2.y, c2.z, r.n);
	length[p] = r.n;
	if(RECTIFY) kept[p] = r.kept;
}
inline LaunchShape merge_launch(int width, int height) { return image_launch(width, height); }

// ---- rectifying stale history: the window statistics ----
// the planes of the staged tile, one float per pixel each: X0 = (D0.rgb, V0), the normal, the point, the albedo, the hit flag
enum RectifyPlane { kPlaneR, kPlaneG, kPlaneB, kPlaneV, kPlaneNx, kPlaneNy, kPlaneNz, kPlanePx, kPlanePy, kPlanePz, kPlaneAr, kPlaneAg, kPlaneAb, kPlaneHit, kRectifyPlanes };
struct RectifyOrigin { float o[3]; };

// One pixel per thread, the workgroup of k_atrous.  (2 R + 1)^2 taps x 64 B per pixel would be read from the images; instead the workgroup stages its
// 32 x 8 pixels with their halo of R once in LDS — (32 + 2 R) x (8 + 2 R) pixels, 532 at R = 3: 2.1 x the tile's own pixels, four 16-byte loads each,
// neighbouring lanes neighbouring pixels — as kRectifyPlanes planes of floats (29 792 B at R = 3), so that for one tap the 32 lanes of a row read 32
// consecutive words of a plane (ds_read_b32 serves lanes 0-31 and 32-63 in a cycle each: no bank conflict; a float4 per pixel would be read 16 lanes
// at a time, 64 B apart: 4-way).  A tile pixel outside the image is staged as zeros: its hit flag refuses it, as the definition skips it.  Every thread
// visits its taps row by row, dy outside and dx inside, through rectify_tap: the sums are the definition's to the bit.  The loops unroll (R is the
// instance's): every LDS address is the centre's plus a constant, the sums stay in registers, no scratch.  Writes R0 and R1, 32 B per pixel.
template <int R>
__global__ __launch_bounds__(kAtrousX * kAtrousY) void k_rectify_window(const float4 *__restrict__ x0, const float4 *__restrict__ x1, const float4 *__restrict__ x2,
                                                                         const float4 *__restrict__ xa, float4 *__restrict__ r0, float4 *__restrict__ r1, int width, int height,
                                                                         RectifyOrigin origin)
{
	constexpr int TW = kAtrousX + 2 * R, TH = kAtrousY + 2 * R, TP = TW * TH;
	__shared__ float tile[kRectifyPlanes][TP];
	const int tid = threadIdx.y * kAtrousX + threadIdx.x;
	const int gx0 = blockIdx.x * kAtrousX - R, gy0 = blockIdx.y * kAtrousY - R;
	for(int i = tid; i < TP; i += kAtrousX * kAtrousY)
	{
		const int ty = i / TW, tx = i - ty * TW;
		const int gx = gx0 + tx, gy = gy0 + ty;
		float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a, d = a;
		if(gx >= 0 && gy >= 0 && gx < width && gy < height)
		{
			const size_t q = (size_t)gy * width + gx;
			a = x0[q]; b = x1[q]; c = x2[q]; d = xa[q];
		}
		tile[kPlaneR][i] = a.x; tile[kPlaneG][i] = a.y; tile[kPlaneB][i] = a.z; tile[kPlaneV][i] = a.w;
		tile[kPlaneNx][i] = b.x; tile[kPlaneNy][i] = b.y; tile[kPlaneNz][i] = b.z; tile[kPlaneHit][i] = b.w;
		tile[kPlanePx][i] = c.x; tile[kPlanePy][i] = c.y; tile[kPlanePz][i] = c.z;
		tile[kPlaneAr][i] = d.x; tile[kPlaneAg][i] = d.y; tile[kPlaneAb][i] = d.z;
	}
	__syncthreads();
	const int x = blockIdx.x * kAtrousX + threadIdx.x, y = blockIdx.y * kAtrousY + threadIdx.y;
	if(x >= width || y >= height) return;
	const int at = (threadIdx.y + R) * TW + threadIdx.x + R; // the centre in the tile; a tap is at + dy * TW + dx, inside the tile for |dx|, |dy| <= R
	RectifySums s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
	if(tile[kPlaneHit][at] != 0.0f)
	{
		const RectifyCentre ctr = rectify_centre(Dn4{tile[kPlaneNx][at], tile[kPlaneNy][at], tile[kPlaneNz][at], 1.0f}, Dn4{tile[kPlanePx][at], tile[kPlanePy][at], tile[kPlanePz][at], 0.0f},
		                                         Dn4{tile[kPlaneAr][at], tile[kPlaneAg][at], tile[kPlaneAb][at], 0.0f}, origin.o);
#pragma unroll
		for(int dy = -R; dy <= R; ++dy)
#pragma unroll
			for(int dx = -R; dx <= R; ++dx)
			{
				const int q = at + dy * TW + dx;
				rectify_tap(ctr, s, tile[kPlaneNx][q], tile[kPlaneNy][q], tile[kPlaneNz][q], tile[kPlaneHit][q], tile[kPlanePx][q], tile[kPlanePy][q], tile[kPlanePz][q], tile[kPlaneAr][q],
				            tile[kPlaneAg][q], tile[kPlaneAb][q], tile[kPlaneR][q], tile[kPlaneG][q], tile[kPlaneB][q], tile[kPlaneV][q]);
			}
	}
	const RectifyStats st = rectify_finish(s);
	const size_t p = (size_t)y * width + x;
	r0[p] = make_float4(st.r0.x, st.r0.y, st.r0.z, st.r0.w);
	r1[p] = make_float4(st.r1.x, st.r1.y, st.r1.z, st.r1.w);
}
inline LaunchShape window_launch(int width, int height) { return image_launch(width, height); }

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
inline LaunchShape snapshot_launch(int64_t n_tris) { return LaunchShape{dim3((unsigned)((n_tris + kSnapshotGroup - 1) / kSnapshotGroup)), dim3(kSnapshotGroup * kSnapshotVecs)}; }

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
__global__ __launch_bounds__(kPixelThreads) void k_motion_gather(const float4 *__restrict__ g_hits, const float4 *__restrict__ g_normal, const float4 *__restrict__ g_position,
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
inline LaunchShape gather_launch(int n_px) { return local_pixels_launch(n_px); }

}  // namespace
