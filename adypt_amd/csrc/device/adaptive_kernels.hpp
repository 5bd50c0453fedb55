// The kernels of adaptive sampling (active_blocks.hpp): they run only while blocks are frozen.  All three are TEMPLATES whose first use lies behind
// the first use of every other kernel template of tracer.hip (frame_schedule.hpp's launch_resolve, then freeze_blocks and query_noise_blocks): the
// compiler emits implicit instantiations behind the plain kernels, in the order of their first use, so these three are the last functions of the
// code object and every kernel the library had keeps its text, its function ordinal and its place ("Noise statistics").
// Two of them restate a kernel of shade.hpp with one index or one count changed.  A body shared with k_resolve_noise / k_noise_blocks was built: it
// changed those two kernels' instructions (a compare and a branch inverted; an address computed in another order), and their text is to stay the
// parent's — so the arithmetic is written out here a second time, and tests/test_gpu_adaptive.py holds both against the same truth bit for bit.
#pragma once
#include "shade.hpp"

namespace adypt {

// dst[P] = src[slot[P >> 10] * 1024 + (P & 1023)] for the n_px = active blocks x 1024 pass-local pixels P: the compact copy of a per-pixel image
// for the active list (the shift image, 2 bytes per pixel: T = uint16_t), rebuilt whenever the set changes.  slot[] < owned blocks (ActiveBlocks::slot).
template <class T> __global__ __launch_bounds__(256) void k_gather_blocks(const T *src, const int32_t *slot, T *dst, int n_px)
{
	const int P = blockIdx.x * blockDim.x + threadIdx.x;
	if(P >= n_px) return;
	dst[P] = src[(size_t)slot[P >> 10] * kBlockPixels + (size_t)(P & 1023)];
}

// k_resolve_noise of a pass over a shrunken block set: f.n_local_px, sc.local_blocks and done[] are the pass's (active blocks), accum and the
// moments stay in owned-block order — pass-local pixel P is owned pixel slot[P >> 10] * 1024 + (P & 1023).  The same arithmetic in the same order.
// (MOMENTS: blocks freeze only with the noise statistics on — there is no variant without.)
template <bool MOMENTS> __global__ __launch_bounds__(256) void k_resolve_noise_slots(FrameArgs f, SceneArgs sc, PixelArgs px, NoiseMoments *moments, const int32_t *slot, int first, int count)
{
	static_assert(MOMENTS, "blocks freeze only with the noise statistics on");
	const int P = blockIdx.x * blockDim.x + threadIdx.x;
	int x, y;
	if(P >= f.n_local_px || !local_pixel_xy(f, sc.local_blocks, P, &x, &y)) return;
	const size_t L = (size_t)slot[P >> 10] * kBlockPixels + (size_t)(P & 1023);
	float4 acc = px.accum[L];
	NoiseMoments m = f.spp + first == 0 ? NoiseMoments{0.0f, 0.0f} : moments[L];
	for(int k = first; k < first + count; ++k)
	{
		const float4 r = f.done[(size_t)k * f.n_local_px + P];
		const float fs = (float)(f.spp + k), fs1 = (float)(f.spp + k + 1);
		acc = make_float4(fmaf(acc.x, fs, r.x) / fs1, fmaf(acc.y, fs, r.y) / fs1, fmaf(acc.z, fs, r.z) / fs1, 1.0f);
		m = noise_add_sample(m, f.spp + k, r.x, r.y, r.z);
	}
	px.accum[L] = acc;
	moments[L] = m;
}

// k_noise_blocks with a sample count per owned block: frozen_at[b] != 0 = owned block b stopped at that many frames, else it holds `spp`.  The
// formulas and the order of the additions are k_noise_blocks'.  (PER_BLOCK: the variant with one count for all is k_noise_blocks.)
template <bool PER_BLOCK> __global__ __launch_bounds__(256) void k_noise_blocks_spp(const NoiseMoments *moments, const int32_t *local_blocks, int blocks_x, int width, int height, int spp,
                                                                                   const int32_t *frozen_at, NoiseBlock *out, float *e_out)
{
	static_assert(PER_BLOCK, "k_noise_blocks is the kernel with one sample count");
	__shared__ double wave_sum[4];
	__shared__ uint32_t wave_count[4];
	const int blk = local_blocks[blockIdx.x];
	const int at = frozen_at[blockIdx.x], n = at ? at : spp;
	double sum = 0.0;
	uint32_t count = 0;
#pragma unroll
	for(int j = 0; j < kBlockPixels / 256; ++j)
	{
		const int in = j * 256 + (int)threadIdx.x;
		const size_t L = (size_t)blockIdx.x * kBlockPixels + in;
		int x, y;
		block_pixel_xy(blk, in, blocks_x, &x, &y);
		const bool inside = x < width && y < height;
		const float e = inside ? noise_of_pixel(moments[L], n) : 0.0f;
		if(inside) { sum += (double)e; ++count; }
		if(e_out) e_out[L] = e;
	}
#pragma unroll
	for(int d = 1; d < 64; d <<= 1) { sum += __shfl_xor(sum, d); count += __shfl_xor(count, d); }
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if(lane == 0) { wave_sum[wave] = sum; wave_count[wave] = count; }
	__syncthreads();
	if(threadIdx.x == 0)
	{
		NoiseBlock b;
		b.sum = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
		b.count = ((wave_count[0] + wave_count[1]) + wave_count[2]) + wave_count[3];
		b.pad = 0u;
		out[blockIdx.x] = b;
	}
}

}  // namespace adypt
