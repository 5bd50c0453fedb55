// The noise estimate: how converged the accumulated image is, per pixel, per 32x32 block and as one number.  THE definition for host and device
// (no HIP needed: a host compiler may include it; tests/test_noise_definition.py does, with -ffp-contract=off).  Canonical arithmetic as in
// canon_math.hpp: binary32, round to nearest, the operations in the order written, and NO fma anywhere in this header — a numpy float32
// restatement of these lines is bit-exact.
//
// Per pixel the luminance Y of every clamped sample that the running mean takes in is folded, in frame order, into (mean, m2) by Welford's
// update; k_resolve<true, *> (shade.hpp) does that next to the running mean, k_noise_blocks turns the moments into numbers when somebody asks.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#ifndef ADYPT_HOST_DEVICE
#ifdef __HIPCC__
#define ADYPT_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define ADYPT_HOST_DEVICE inline
#endif
#endif

namespace adypt {

// state per local pixel; (0, 0) when the image is cleared
struct NoiseMoments { float mean, m2; };

// what a block contributes: the sum of its pixels' noise (binary64) over the `count` pixels of the block that lie inside the image
struct NoiseBlock { double sum; uint32_t count; uint32_t pad; };

constexpr float kNoiseBlackLevel = 0.01f; // keeps black pixels finite; part of the definition, not a tunable

ADYPT_HOST_DEVICE float noise_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// sample (r, g, b) of the frame with 0-based index k of the accumulation
ADYPT_HOST_DEVICE NoiseMoments noise_add_sample(NoiseMoments s, int k, float r, float g, float b)
{
	const float n = (float)(k + 1);
	const float y = noise_luminance(r, g, b);
	const float d = y - s.mean;
	s.mean = s.mean + d / n;
	s.m2 = s.m2 + d * (y - s.mean); // (with the NEW mean)
	return s;
}

// relative standard error of the mean luminance after n_frames >= 2 frames
ADYPT_HOST_DEVICE float noise_of_pixel(NoiseMoments s, int n_frames)
{
	const float n = (float)n_frames;
	return sqrtf(s.m2 / (n * (n - 1.0f))) / (s.mean + kNoiseBlackLevel);
}

// THE host record of one 32x32 block of an image: what k_noise_blocks found for it (sum, count), which block of the image it is, the frames it holds
// and whether it is frozen at them (active_blocks.hpp).  Every host-side consumer reads blocks in this shape; the C ABI's parallel arrays are
// filled from it at the boundary.
struct BlockState { int32_t index; double sum; uint32_t count; int32_t spp; bool frozen; };

// The image's numbers from its blocks' (host only).  blocks[0 .. n_blocks): ascending index; `pixels` = the pixels the entries cover (width x height
// for a whole image).  mean_noise = (sum of the block sums, in that order) / pixels; worst_block = the largest sum / count, worst_index its block
// index — the lowest one on a tie.  Entries without a pixel (count 0) are passed over.  Nothing covered: zeros.
struct NoiseImage { double mean_noise, worst_block; int32_t worst_index; };
inline NoiseImage noise_of_image(const BlockState *blocks, size_t n_blocks, int64_t pixels)
{
	NoiseImage r{0.0, 0.0, 0};
	double total = 0.0;
	bool any = false;
	for(size_t i = 0; i < n_blocks; ++i)
	{
		const BlockState &b = blocks[i];
		if(b.count == 0) continue;
		total += b.sum;
		const double m = b.sum / (double)b.count;
		if(!any || m > r.worst_block) { r.worst_block = m; r.worst_index = b.index; any = true; }
	}
	if(any && pixels > 0) r.mean_noise = total / (double)pixels;
	return r;
}

}  // namespace adypt
