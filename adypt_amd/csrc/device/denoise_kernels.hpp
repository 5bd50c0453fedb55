// The denoiser's kernels and the shape each is launched with, in a header of their own so that two libraries compile the same text: denoise.hip, which
// is the product, and csrc/probe/probe.hip, which runs every kernel on arrays a test makes (tests/test_gpu_denoise_probes.py).  The kernels stay in the
// anonymous namespace: each including unit has its own copies, and nothing here is visible outside it.  Who launches a kernel takes the grid and the
// workgroup from the *_launch function beside it — denoise.hip and the probe alike — so that the probe's launch shape cannot drift from the product's; the instance of a
// templated kernel likewise, from the *_instance functions at the end.
// What the stages are and in which order they run: the head of denoise.hip.
#pragma once
#include "tile_layout.hpp"
#include "denoise.hpp"
#include "temporal.hpp"
#include "guide_chain.hpp"
#include "texture.hpp"

#include <hip/hip_runtime.h>

namespace {

using namespace adypt;

struct LaunchShape { dim3 grid, block; };

constexpr int kPixelThreads = 256; // the workgroup of the kernels that run one thread per local pixel of a block list: prepare and gather

// one thread per local pixel of a block list of n_px local pixels
inline LaunchShape local_pixels_launch(int n_px) { return LaunchShape{dim3((unsigned)(((int64_t)n_px + kPixelThreads - 1) / kPixelThreads)), dim3(kPixelThreads)}; }

// CLASS: X1.w is the class code the chain through mirrors and glass left in the .w of the primary-hit image (k_chain_start, k_chain_step) instead of the
// hit flag: adypt_denoise_specular's instance, k_denoise_prepare_class.  The other instance is what k_denoise_prepare was before there was a chain.
// MOMENTS: X0.w = S0, the raw second moment of moments.hpp, defined from 1 spp: a moments call's instance, k_denoise_prepare_moments.
template <bool CLASS, bool MOMENTS = false>
__device__ __forceinline__ void denoise_prepare_pixel(const float4 *accum, const float2 *moments, const int32_t *blocks, const int32_t *block_spp, int n_px, int blocks_x, int width, int height,
                                                      const float4 *g_albedo, const float4 *g_normal, const float4 *g_position, const float4 *g_hits, float4 *x0, float4 *x1, float4 *x2,
                                                      float4 *xa)
{
	const int L = blockIdx.x * blockDim.x + threadIdx.x;
	if(L >= n_px) return;
	int x, y;
	block_pixel_xy(blocks[L >> 10], L & 1023, blocks_x, &x, &y);
	if(x >= width || y >= height) return; // (blocks at the right and bottom edge stick out)
	const size_t p = (size_t)y * width + x;
	const float4 c = accum[L], a = g_albedo[L], n = g_normal[L], q = g_position[L];
	const Dn4 d = MOMENTS ? moments_prepare(c.x, c.y, c.z, moments[L].y, (float)block_spp[L >> 10], a.x, a.y, a.z)
	                      : denoise_prepare(c.x, c.y, c.z, moments[L].y, (float)block_spp[L >> 10], a.x, a.y, a.z);
	x0[p] = make_float4(d.x, d.y, d.z, d.w);
	x1[p] = make_float4(n.x, n.y, n.z, CLASS ? g_hits[L].w : (__float_as_int(g_hits[L].x) != -1 ? 1.0f : 0.0f));
	x2[p] = make_float4(q.x, q.y, q.z, (float)block_spp[L >> 10]); // (.w: the sample count, which only the temporal merge reads)
	xa[p] = make_float4(a.x, a.y, a.z, 0.0f);
}
__global__ __launch_bounds__(kPixelThreads) void k_denoise_prepare(const float4 *accum, const float2 *moments, const int32_t *blocks, const int32_t *block_spp, int n_px, int blocks_x, int width,
                                                                   int height, const float4 *g_albedo, const float4 *g_normal, const float4 *g_position, const float4 *g_hits, float4 *x0,
                                                                   float4 *x1, float4 *x2, float4 *xa)
{
	denoise_prepare_pixel<false>(accum, moments, blocks, block_spp, n_px, blocks_x, width, height, g_albedo, g_normal, g_position, g_hits, x0, x1, x2, xa);
}
__global__ __launch_bounds__(kPixelThreads) void k_denoise_prepare_class(const float4 *accum, const float2 *moments, const int32_t *blocks, const int32_t *block_spp, int n_px, int blocks_x,
                                                                         int width, int height, const float4 *g_albedo, const float4 *g_normal, const float4 *g_position, const float4 *g_hits,
                                                                         float4 *x0, float4 *x1, float4 *x2, float4 *xa)
{
	denoise_prepare_pixel<true>(accum, moments, blocks, block_spp, n_px, blocks_x, width, height, g_albedo, g_normal, g_position, g_hits, x0, x1, x2, xa);
}
__global__ __launch_bounds__(kPixelThreads) void k_denoise_prepare_moments(const float4 *accum, const float2 *moments, const int32_t *blocks, const int32_t *block_spp, int n_px, int blocks_x,
                                                                           int width, int height, const float4 *g_albedo, const float4 *g_normal, const float4 *g_position, const float4 *g_hits,
                                                                           float4 *x0, float4 *x1, float4 *x2, float4 *xa)
{
	denoise_prepare_pixel<false, true>(accum, moments, blocks, block_spp, n_px, blocks_x, width, height, g_albedo, g_normal, g_position, g_hits, x0, x1, x2, xa);
}
// k_denoise_prepare_class that also brings the virtual point to the picture's coordinates (adypt_denoise_temporal_specular): g_virtual is the block-major
// image k_chain_step<true> wrote for the pixels whose chain ended on a surface, which are the pixels of class >= 2 and the only ones it is read at;
// XV = (Pv.xyz, len) there and (P, 0) everywhere else — THE rule of who has a virtual point (guide_chain.hpp), stated here once.  16 B per pixel more
// written, and 16 B more read at a followed pixel.
__global__ __launch_bounds__(kPixelThreads) void k_denoise_prepare_virtual(const float4 *accum, const float2 *moments, const int32_t *blocks, const int32_t *block_spp, int n_px, int blocks_x,
                                                                           int width, int height, const float4 *g_albedo, const float4 *g_normal, const float4 *g_position, const float4 *g_hits,
                                                                           float4 *x0, float4 *x1, float4 *x2, float4 *xa, const float4 *g_virtual, float4 *xv)
{
	denoise_prepare_pixel<true>(accum, moments, blocks, block_spp, n_px, blocks_x, width, height, g_albedo, g_normal, g_position, g_hits, x0, x1, x2, xa);
	const int L = blockIdx.x * blockDim.x + threadIdx.x;
	if(L >= n_px) return;
	int x, y;
	block_pixel_xy(blocks[L >> 10], L & 1023, blocks_x, &x, &y);
	if(x >= width || y >= height) return;
	const float4 q = g_position[L];
	xv[(size_t)y * width + x] = g_hits[L].w >= 2.0f ? g_virtual[L] : make_float4(q.x, q.y, q.z, 0.0f);
}
inline LaunchShape prepare_launch(int n_px) { return local_pixels_launch(n_px); }

// ---- the chain through mirrors and glass (guide_chain.hpp) ----
// What the chain's kernels read of the scene, the guide scratch they finish pixels in, the queue they append rays to, what they count.
struct ChainScene { const float4 *triangles, *materials; const uint32_t *texels; int64_t n_tris; int32_t n_mats, n_tex; };
struct ChainGuides { float4 *albedo, *normal, *position, *hits; }; // block-major, one float4 per local pixel; hits.w takes the class
struct ChainQueue { float4 *o, *d; uint32_t *count; uint32_t seg_cap, seg_stride; int segments; }; // count[s * seg_stride]: the rays of segment s
struct ChainCounts { unsigned long long rays, followed, escaped, truncated; };
struct ChainOrigin { float o[3]; float tmin; };

// the material of triangle `tri` for the chain; want_kd: with the diffuse colour the shading would take at (u, v), the texture's where there is one
__device__ __forceinline__ ChainMaterial chain_material(const ChainScene &sc, int tri, float u, float v, bool want_kd)
{
	ChainMaterial m{true, 0, Ch3{0.0f, 0.0f, 0.0f}, Ch3{0.0f, 0.0f, 0.0f}, 1.0f};
	const int matid = __float_as_int(sc.triangles[(size_t)tri * kTriFloat4 + 4].z);
	if(matid < 0 || matid >= sc.n_mats) return m;
	const float4 *mp = sc.materials + (size_t)matid * kMatFloat4;
	const float4 md = mp[0], ms = mp[2], mx = mp[3];
	m.bad = false; m.illum = __float_as_int(mx.x); m.ior = mx.w;
	m.ks = Ch3{ms.y, ms.z, ms.w};
	m.kd = Ch3{md.y, md.z, md.w};
	const int dtex = __float_as_int(md.x);
	if(want_kd && !chain_is_delta(false, m.illum) && sc.n_tex != 0 && dtex != -1 && dtex >= 0 && dtex < sc.n_tex)
	{
		const float4 mt = mp[4];
		const SceneArgs scene{sc.triangles, sc.materials, sc.texels, nullptr, nullptr};
		const F3 c = textured_diffuse(scene, tri, make_int4(__float_as_int(mt.x), __float_as_int(mt.y), __float_as_int(mt.z), 0), u, v, 1.0f - u - v);
		m.kd = Ch3{c.x, c.y, c.z};
	}
	return m;
}

// A wave's survivors take consecutive slots of the segment: the vote, the lane's rank among the voters (v_mbcnt), ONE atomic per wave by the first
// voter, its answer read by the others.  The vote is taken once and nothing waits between it and its use: no mask crosses a barrier.
// Every lane of the wave calls this.  Returns the slot inside the segment (valid where `alive`).
__device__ __forceinline__ uint32_t chain_append(bool alive, uint32_t *seg_counter)
{
	const unsigned long long mask = __ballot(alive);
	const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
	uint32_t base = 0u;
	if(alive && rank == 0u) base = atomicAdd(seg_counter, (uint32_t)__popcll(mask));
	const int first = mask ? __ffsll((long long)mask) - 1 : 0;
	return (uint32_t)__shfl((int)base, first) + rank;
}
// a count of the lanes that say `yes`: one atomic per wave
__device__ __forceinline__ void chain_count(bool yes, unsigned long long *counter)
{
	const unsigned long long mask = __ballot(yes);
	const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
	if(yes && rank == 0u) atomicAdd(counter, (unsigned long long)__popcll(mask));
}

// (len: the unfolded length of the unfolding instances, which travels in the free word; the others leave it 0)
__device__ __forceinline__ void chain_store_state(float4 *state, int L, const ChainState &s, float len = 0.0f)
{
	state[2 * (size_t)L] = make_float4(s.t.x, s.t.y, s.t.z, __int_as_float(s.length));
	state[2 * (size_t)L + 1] = make_float4(s.d.x, s.d.y, s.d.z, len);
}
// what the unfolding instances are given beside the others' arguments: the block-major image of the virtual points, one float4 per local pixel, written
// where a chain ends on a surface — (Pv.xyz, valid ? len : 0) — and nowhere else
struct ChainUnfold { float4 *virt; float o[3]; }; // (o: the camera origin)
__device__ __forceinline__ void chain_store_ray(const ChainQueue &q, uint32_t seg, uint32_t in_seg, const Ch3 &p, const Ch3 &d, float tmin, int L)
{
	if(in_seg >= q.seg_cap) return; // (the host sizes the launch so that a segment cannot overflow; never write outside one)
	const size_t slot = (size_t)seg * q.seg_cap + in_seg;
	q.o[slot] = make_float4(p.x, p.y, p.z, tmin);
	q.d[slot] = make_float4(d.x, d.y, d.z, __int_as_float(L)); // (the local pixel travels in .w, as in the sun-visibility queue)
}

// One thread per local pixel of the owned block list, behind the guide capture.  Reads the primary hit (16 B) and, where it is a hit, the material
// (48 B of its record, 16 B of the triangle's) and the normal and position guides (32 B); writes the class of a pixel that is not followed into the .w
// of its hit (4 B), else the pixel's state (32 B) and a ray (32 B).  Workgroup b appends to segment b % segments: 256 rays at most each.
// UNFOLD (adypt_denoise_temporal_specular's instance): the state also takes the length of the camera ray, chain_start_length — one square root more
// per followed pixel.  The kernel itself is the template, with no body shared through a call: k_chain_start<false> is what k_chain_start was.
template <bool UNFOLD>
__global__ __launch_bounds__(kPixelThreads) void k_chain_start(ChainScene sc, ChainGuides g, const int32_t *__restrict__ blocks, int n_px, int blocks_x, int width, int height,
                                                               ChainOrigin origin, int bounces, float4 *__restrict__ state, ChainQueue out, ChainCounts *counts)
{
	const int L = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t seg = blockIdx.x % (uint32_t)out.segments;
	bool go = false;
	ChainState s{Ch3{1.0f, 1.0f, 1.0f}, Ch3{0.0f, 0.0f, 0.0f}, 0};
	Ch3 p{0.0f, 0.0f, 0.0f};
	if(L < n_px)
	{
		int x, y;
		block_pixel_xy(blocks[L >> 10], L & 1023, blocks_x, &x, &y);
		if(x < width && y < height)
		{
			const float4 hq = g.hits[L];
			const int32_t tri = __float_as_int(hq.x);
			if(tri >= 0 && (int64_t)tri < sc.n_tris)
			{
				const ChainMaterial m = chain_material(sc, tri, hq.y, hq.z, false);
				const float4 n = g.normal[L], q = g.position[L];
				p = Ch3{q.x, q.y, q.z};
				go = chain_at_primary(s, m, Ch3{n.x, n.y, n.z}, p, origin.o, bounces) == kChainGoesOn;
			}
			if(!go) g.hits[L].w = tri != -1 ? 1.0f : 0.0f;
		}
	}
	const uint32_t in_seg = chain_append(go, out.count + seg * out.seg_stride);
	if(go)
	{
		chain_store_state(state, L, s, UNFOLD ? chain_start_length(p, origin.o) : 0.0f);
		chain_store_ray(out, seg, in_seg, p, s.d, origin.tmin, L);
	}
	chain_count(go, &counts->followed);
	chain_count(go, &counts->rays);
}
inline LaunchShape chain_start_launch(int n_px) { return local_pixels_launch(n_px); }

// One thread per traced ray: workgroup b takes rays [256 (b / segments), ...) of segment b % segments of the queue the traversal has just answered.
// Reads the ray's direction word and hit (32 B), the pixel's state (32 B) and at a hit 80 B of the triangle's record, 48 B of the material's and, on a
// textured surface that ends the chain, 16 B of texture coordinates and 4 texels; either ends the pixel — albedo, normal, position (48 B) and the class
// into the .w of its hit (4 B) — or writes the state back and appends the next ray to the same segment of the other queue (64 B).
// UNFOLD (adypt_denoise_temporal_specular's instance): also reads the origin of the ray from the queue it consumes (16 B) and adds the ray's length to the state's
// (chain_unfold); a pixel that ends on a surface reads the primary position guide, which it still finds in place before it overwrites it, and writes
// its virtual point (chain_virtual_point; 16 B) — one square root and one 16-byte load more per step.  It appends to the queue as the other does.  The
// kernel itself is the template; `unfold` stands last and k_chain_step<false> never looks at it: its code is what k_chain_step's was.
template <bool UNFOLD>
__global__ __launch_bounds__(kPixelThreads) void k_chain_step(ChainScene sc, ChainGuides g, ChainQueue in, const float4 *__restrict__ hit, int n_px, int bounces, float tmin,
                                                              float4 *__restrict__ state, ChainQueue out, ChainCounts *counts, ChainUnfold unfold)
{
	const uint32_t seg = blockIdx.x % (uint32_t)in.segments, local = (blockIdx.x / (uint32_t)in.segments) * kPixelThreads + threadIdx.x;
	const uint32_t n_in = min(in.count[seg * in.seg_stride], in.seg_cap);
	bool go = false, escaped = false, truncated = false;
	ChainState s{Ch3{1.0f, 1.0f, 1.0f}, Ch3{0.0f, 0.0f, 0.0f}, 0};
	Ch3 p{0.0f, 0.0f, 0.0f};
	float len = 0.0f;
	int L = -1;
	if(local < n_in)
	{
		const size_t slot = (size_t)seg * in.seg_cap + local;
		L = __float_as_int(in.d[slot].w);
		if(L < 0 || L >= n_px) L = -1; // (never an index that is none)
	}
	if(L >= 0)
	{
		const size_t slot = (size_t)seg * in.seg_cap + local;
		const float4 h = hit[slot], s0 = state[2 * (size_t)L], s1 = state[2 * (size_t)L + 1];
		s = ChainState{Ch3{s0.x, s0.y, s0.z}, Ch3{s1.x, s1.y, s1.z}, __float_as_int(s0.w)};
		const int32_t tri = __float_as_int(h.x);
		ChainEnd end;
		if(tri < 0 || (int64_t)tri >= sc.n_tris) { end = chain_escaped(s); escaped = true; }
		else
		{
			s.length = s.length + 1;
			float w[20]; // words 0..17 of the record: positions and normals (indexed by constants after unrolling: registers)
			const float4 *rec = sc.triangles + (size_t)tri * kTriFloat4;
#pragma unroll
			for(int k = 0; k < 5; ++k)
			{
				const float4 v = rec[k];
				w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
			}
			Ch3 n;
			chain_hit_point(w, h.y, h.z, &p, &n);
			if(UNFOLD)
			{
				const float4 ro = in.o[slot];
				len = chain_unfold(s1.w, p, Ch3{ro.x, ro.y, ro.z});
			}
			const ChainMaterial m = chain_material(sc, tri, h.y, h.z, true);
			go = chain_at_surface(s, m, n, p, bounces, &end) == kChainGoesOn;
			truncated = !go && chain_is_delta(m.bad, m.illum);
		}
		if(!go)
		{
			if(UNFOLD && !escaped)
			{
				const float4 q0 = g.position[L]; // (the primary capture's: this thread is the first to overwrite it, below)
				const ChainVirtual v = chain_virtual_point(Ch3{q0.x, q0.y, q0.z}, unfold.o, len);
				unfold.virt[L] = make_float4(v.p.x, v.p.y, v.p.z, v.valid ? len : 0.0f);
			}
			g.albedo[L] = make_float4(end.albedo.x, end.albedo.y, end.albedo.z, 1.0f);
			g.normal[L] = make_float4(end.normal.x, end.normal.y, end.normal.z, 1.0f);
			g.position[L] = make_float4(end.position.x, end.position.y, end.position.z, 1.0f);
			g.hits[L].w = (float)end.cls;
		}
	}
	const uint32_t in_seg = chain_append(go, out.count + seg * out.seg_stride);
	if(go)
	{
		chain_store_state(state, L, s, len);
		chain_store_ray(out, seg, in_seg, p, s.d, tmin, L);
	}
	chain_count(go, &counts->rays);
	chain_count(escaped, &counts->escaped);
	chain_count(truncated, &counts->truncated);
}

// rays_per_segment: the most rays a segment can hold in any round = 256 x the workgroups of k_chain_start that append to it
inline LaunchShape chain_step_launch(int segments, uint32_t rays_per_segment) { return LaunchShape{dim3((unsigned)segments * ((rays_per_segment + kPixelThreads - 1) / kPixelThreads)), dim3(kPixelThreads)}; }

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
// instances without it pass temporal_merge a constant "off": their code is what it was.  MOMENTS (k_temporal_merge_moments, below): the fourth channel of
// X0, of the history and of the merged image is the raw second moment S (moments.hpp), blended with w; same bytes, never together with RECTIFY.
template <bool MOTION, bool RECTIFY, bool MOMENTS>
__device__ __forceinline__ void temporal_merge_pixel(const float4 *x0, const float4 *x1, float4 *x2, const float4 *xa, const float4 *h0, const float4 *h1, const float4 *h2, const float4 *ha,
                                                     float4 *merged, float *length, int width, int height, int have, const TemporalCamera &cam, float history_cap, const float4 *xp,
                                                     const float4 *xn, const float4 *r0, const float4 *r1, float *kept, float gamma)
{
	const int x = blockIdx.x * kAtrousX + threadIdx.x, y = blockIdx.y * kAtrousY + threadIdx.y;
	if(x >= width || y >= height) return;
	const int p = y * width + x;
	const Dn4 c2 = DeviceImages::load(x2, p);
	const DeviceHistory hist{h0, h1, h2, ha};
	Rectify rect;
	if(RECTIFY) rect = Rectify{true, DeviceImages::load(r0, p), DeviceImages::load(r1, p), gamma};
	const TemporalOut r = MOTION ? temporal_merge_motion<MOMENTS>(hist, have != 0, cam, width, height, DeviceImages::load(x0, p), DeviceImages::load(x1, p), DeviceImages::load(xa, p), c2.w, history_cap,
	                                                     DeviceImages::load(xp, p), DeviceImages::load(xn, p), rect)
	                             : temporal_merge<MOMENTS>(hist, have != 0, cam, width, height, DeviceImages::load(x0, p), DeviceImages::load(x1, p), c2, DeviceImages::load(xa, p), c2.w, history_cap, rect);
	merged[p] = make_float4(r.x0.x, r.x0.y, r.x0.z, r.x0.w);
	x2[p] = make_float4(c2.x, c2.y, c2.z, r.n);
	length[p] = r.n;
	if(RECTIFY) kept[p] = r.kept;
}
template <bool MOTION, bool RECTIFY>
__global__ __launch_bounds__(kAtrousX * kAtrousY) void k_temporal_merge(const float4 *x0, const float4 *x1, float4 *x2, const float4 *xa, const float4 *h0, const float4 *h1,
                                                                         const float4 *h2, const float4 *ha, float4 *merged, float *length, int width, int height, int have,
                                                                         TemporalCamera cam, float history_cap, const float4 *xp, const float4 *xn, const float4 *r0, const float4 *r1, float *kept,
                                                                         float gamma)
{
	temporal_merge_pixel<MOTION, RECTIFY, false>(x0, x1, x2, xa, h0, h1, h2, ha, merged, length, width, height, have, cam, history_cap, xp, xn, r0, r1, kept, gamma);
}
// a moments call's merge: k_temporal_merge<MOTION, false>'s arguments without the rectified call's
template <bool MOTION>
__global__ __launch_bounds__(kAtrousX * kAtrousY) void k_temporal_merge_moments(const float4 *x0, const float4 *x1, float4 *x2, const float4 *xa, const float4 *h0, const float4 *h1,
                                                                                 const float4 *h2, const float4 *ha, float4 *merged, float *length, int width, int height, int have,
                                                                                 TemporalCamera cam, float history_cap, const float4 *xp, const float4 *xn)
{
	temporal_merge_pixel<MOTION, false, true>(x0, x1, x2, xa, h0, h1, h2, ha, merged, length, width, height, have, cam, history_cap, xp, xn, nullptr, nullptr, nullptr, 0.0f);
}
// The merge by the virtual point (temporal.hpp temporal_merge_virtual): k_temporal_merge<false, false>'s workgroup, one pixel per thread, and its bytes with
// XV beside the call's images (16 B more read: 180 B per pixel).  It counts the followed pixels (class >= 2) and those of them that took history
// (n_out > n): one atomic per wave and counter as chain_count does, spread over kVirtualCountSlots pairs of counters by workgroup, which the host sums
// (k_moments_variance tells what one address costs).  No thread leaves before the votes: every lane of a wave takes part in them.
constexpr int kVirtualCountSlots = 64;
__global__ __launch_bounds__(kAtrousX * kAtrousY) void k_temporal_merge_virtual(const float4 *x0, const float4 *x1, float4 *x2, const float4 *xa, const float4 *xv, const float4 *h0,
                                                                                 const float4 *h1, const float4 *h2, const float4 *ha, float4 *merged, float *length, int width, int height,
                                                                                 int have, TemporalCamera cam, float history_cap, unsigned long long *counts)
{
	const int x = blockIdx.x * kAtrousX + threadIdx.x, y = blockIdx.y * kAtrousY + threadIdx.y;
	const bool inside = x < width && y < height;
	bool followed = false, with_history = false;
	if(inside)
	{
		const int p = y * width + x;
		const Dn4 c1 = DeviceImages::load(x1, p), c2 = DeviceImages::load(x2, p);
		const DeviceHistory hist{h0, h1, h2, ha};
		const TemporalOut r = temporal_merge_virtual(hist, have != 0, cam, width, height, DeviceImages::load(x0, p), c1, c2, DeviceImages::load(xa, p), DeviceImages::load(xv, p), c2.w, history_cap);
		merged[p] = make_float4(r.x0.x, r.x0.y, r.x0.z, r.x0.w);
		x2[p] = make_float4(c2.x, c2.y, c2.z, r.n);
		length[p] = r.n;
		followed = c1.w >= 2.0f;
		with_history = followed && r.n > c2.w;
	}
	unsigned long long *slot = counts + 2 * ((blockIdx.y * gridDim.x + blockIdx.x) & (kVirtualCountSlots - 1));
	chain_count(followed, slot);
	chain_count(with_history, slot + 1);
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

// ---- variance from temporal moments: the variance the first level sees (moments.hpp) ----
// the planes of the staged tile of the MERGED images, one float per pixel each: lum(D), S, the normal, the point, the albedo, the hit flag
enum MomentsPlane { kMPlaneY, kMPlaneS, kMPlaneNx, kMPlaneNy, kMPlaneNz, kMPlanePx, kMPlanePy, kMPlanePz, kMPlaneAr, kMPlaneAg, kMPlaneAb, kMPlaneHit, kMomentsPlanes };

// One pixel per thread, the workgroup of k_atrous, behind the merge of a moments call.  Reads the merged (D, S) (16 B), the hit flag and n_out (4 B each);
// writes (D, V) into `out` — the first level's source, another image than `merged`, which a commit swaps into the history as it is and whose halo the
// neighbouring workgroups read from global memory — and V into the read-out (4 B): 44 B per pixel.  That is all where no pixel of the workgroup asks its
// window (moments_wants_window: a hit whose history is shorter than kMomentsMinLength), which one workgroup-wide vote decides before anything else is
// loaded: in steady state the workgroups away from what the camera uncovered (53 % of them on the bench orbit).  Where one does, the workgroup stages its 32 x 8 pixels with their halo of 3 in LDS as k_rectify_window
// does — 38 x 14 = 532 pixels, four 16-byte loads each, as kMomentsPlanes planes of floats (25 536 B), lum(D) computed once per staged pixel — and the
// asking threads visit their 49 taps through moments_tap, row by row: the sums are the definition's to the bit.  A tile pixel outside the image is
// staged as zeros: its hit flag refuses it.  The loops unroll: every LDS address is the centre's plus a constant, the sums stay in registers, no scratch.
// The pixels that took the window estimate are counted per workgroup (__syncthreads_count, in the workgroups that staged only: no other has any) and added
// by one thread to one of kMomentsCountSlots counters, which the host sums: one atomic per wave on ONE address measured 0.30 ms of the kernel's 0.44 ms
// at 1920 x 1080 where every pixel is counted (32 400 atomics the L2 serialises; profiles/moments_cost.txt has the figures after the change).
constexpr int kMomentsCountSlots = 64;
__global__ __launch_bounds__(kAtrousX * kAtrousY) void k_moments_variance(const float4 *__restrict__ merged, const float4 *__restrict__ x1, const float4 *__restrict__ x2,
                                                                           const float4 *__restrict__ xa, float4 *__restrict__ out, float *__restrict__ variance,
                                                                           unsigned long long *__restrict__ spatial_count, int width, int height, RectifyOrigin origin)
{
	constexpr int R = kMomentsRadius, TW = kAtrousX + 2 * R, TH = kAtrousY + 2 * R, TP = TW * TH;
	__shared__ float tile[kMomentsPlanes][TP];
	const int x = blockIdx.x * kAtrousX + threadIdx.x, y = blockIdx.y * kAtrousY + threadIdx.y;
	const bool inside = x < width && y < height;
	const size_t p = inside ? (size_t)y * width + x : 0;
	float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	float hit_flag = 0.0f, n_out = 0.0f;
	if(inside) { m = merged[p]; hit_flag = x1[p].w; n_out = x2[p].w; }
	const bool windowed = inside && moments_wants_window(hit_flag != 0.0f, n_out);
	const bool staged = __syncthreads_or(windowed ? 1 : 0) != 0; // (uniform over the workgroup: every thread takes the same side below)
	MomentsSums s{0.0f, 0.0f, 0.0f};
	if(staged)
	{
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
				a = merged[q]; b = x1[q]; c = x2[q]; d = xa[q];
			}
			tile[kMPlaneY][i] = noise_luminance(a.x, a.y, a.z); tile[kMPlaneS][i] = a.w;
			tile[kMPlaneNx][i] = b.x; tile[kMPlaneNy][i] = b.y; tile[kMPlaneNz][i] = b.z; tile[kMPlaneHit][i] = b.w;
			tile[kMPlanePx][i] = c.x; tile[kMPlanePy][i] = c.y; tile[kMPlanePz][i] = c.z;
			tile[kMPlaneAr][i] = d.x; tile[kMPlaneAg][i] = d.y; tile[kMPlaneAb][i] = d.z;
		}
		__syncthreads();
		if(windowed)
		{
			const int at = (threadIdx.y + R) * TW + threadIdx.x + R; // the centre in the tile; a tap is at + dy * TW + dx, inside the tile for |dx|, |dy| <= R
			const RectifyCentre ctr = rectify_centre(Dn4{tile[kMPlaneNx][at], tile[kMPlaneNy][at], tile[kMPlaneNz][at], 1.0f}, Dn4{tile[kMPlanePx][at], tile[kMPlanePy][at], tile[kMPlanePz][at], 0.0f},
			                                         Dn4{tile[kMPlaneAr][at], tile[kMPlaneAg][at], tile[kMPlaneAb][at], 0.0f}, origin.o);
#pragma unroll
			for(int dy = -R; dy <= R; ++dy)
#pragma unroll
				for(int dx = -R; dx <= R; ++dx)
				{
					const int q = at + dy * TW + dx;
					moments_tap(ctr, s, tile[kMPlaneNx][q], tile[kMPlaneNy][q], tile[kMPlaneNz][q], tile[kMPlaneHit][q], tile[kMPlanePx][q], tile[kMPlanePy][q], tile[kMPlanePz][q], tile[kMPlaneAr][q],
					            tile[kMPlaneAg][q], tile[kMPlaneAb][q], tile[kMPlaneY][q], tile[kMPlaneS][q]);
				}
		}
	}
	const MomentsVariance r = moments_finish(moments_own(noise_luminance(m.x, m.y, m.z), m.w), n_out, windowed, s);
	if(staged) // (uniform over the workgroup)
	{
		const int n_spatial = __syncthreads_count(inside && r.spatial ? 1 : 0);
		if(threadIdx.x == 0 && threadIdx.y == 0 && n_spatial > 0)
			atomicAdd(spatial_count + ((blockIdx.y * gridDim.x + blockIdx.x) & (kMomentsCountSlots - 1)), (unsigned long long)n_spatial);
	}
	if(!inside) return;
	out[p] = make_float4(m.x, m.y, m.z, r.v);
	variance[p] = r.v;
}
inline LaunchShape variance_launch(int width, int height) { return image_launch(width, height); }

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

// ---- which instance of a kernel a launch takes ----
// Asked here by denoise.hip and the probe alike, as the launch shapes are.  (Together, and in this order: a unit's code object holds the instances of
// the templates in the order they are first named.)
// the prepare of a call: `moments`, else `followed` (X1.w is the class); k_denoise_prepare_virtual has arguments of its own and no place here
inline decltype(&k_denoise_prepare) prepare_instance(bool moments, bool followed) { return moments ? k_denoise_prepare_moments : followed ? k_denoise_prepare_class : k_denoise_prepare; }
inline decltype(&k_rectify_window<1>) window_instance(int radius)
{
	static_assert(kRectifyMaxRadius == 3, "one instance of k_rectify_window per radius");
	return radius == 1 ? k_rectify_window<1> : radius == 2 ? k_rectify_window<2> : k_rectify_window<3>;
}
inline decltype(&k_temporal_merge<false, false>) merge_instance(bool motion, bool rectify)
{
	return rectify ? (motion ? k_temporal_merge<true, true> : k_temporal_merge<false, true>) : (motion ? k_temporal_merge<true, false> : k_temporal_merge<false, false>);
}
inline decltype(&k_temporal_merge_moments<false>) merge_moments_instance(bool motion) { return motion ? k_temporal_merge_moments<true> : k_temporal_merge_moments<false>; }
inline decltype(&k_atrous<false>) atrous_instance(bool last) { return last ? k_atrous<true> : k_atrous<false>; }
inline decltype(&k_chain_start<false>) chain_start_instance(bool unfold) { return unfold ? k_chain_start<true> : k_chain_start<false>; }
inline decltype(&k_chain_step<false>) chain_step_instance(bool unfold) { return unfold ? k_chain_step<true> : k_chain_step<false>; }

}  // namespace
