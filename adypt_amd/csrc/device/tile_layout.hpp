// The pixel-tile shard: which 32x32 blocks of the image a rank owns, and where pixel `in` of a block lies in the image.  THE definition for host
// and device (no HIP needed: a host compiler may include it).  A context's per-pixel buffers are block-major over its owned blocks: local pixel L
// is pixel L % 1024 of block L / 1024 of the list.  (traverse.hpp's k_trace_camera hoists the same map per wave inside its hot loop.)
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define ADYPT_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define ADYPT_HOST_DEVICE inline
#endif

namespace adypt {

constexpr int kBlockShift = 5;                 // 32x32 pixel shard blocks
constexpr int kBlockDim = 1 << kBlockShift;
constexpr int kBlockPixels = kBlockDim * kBlockDim;

// a block = 4 x 4 wave tiles of 8 x 8 pixels, row-major both ways: 64 consecutive local pixels are one wave's tile
ADYPT_HOST_DEVICE void block_pixel_xy(int blk, int in, int blocks_x, int *x, int *y)
{
	const int wt = in >> 6, ln = in & 63;
	*x = (blk % blocks_x) * kBlockDim + (wt & 3) * 8 + (ln & 7);
	*y = (blk / blocks_x) * kBlockDim + (wt >> 2) * 8 + (ln >> 3);
}

// block ownership: diagonal interleave so that every rank gets sky and floor alike
inline int block_owner(int bx, int by, int nranks) { return (bx + by) % nranks; }

inline std::vector<int32_t> owned_blocks(int width, int height, int rank, int nranks)
{
	const int nbx = (width + kBlockDim - 1) / kBlockDim, nby = (height + kBlockDim - 1) / kBlockDim;
	std::vector<int32_t> v;
	for(int by = 0; by < nby; ++by)
		for(int bx = 0; bx < nbx; ++bx)
			if(block_owner(bx, by, nranks) == rank) v.push_back(by * nbx + bx);
	return v;
}

// f(L, x, y) for every local pixel of the block list that lies inside the image (blocks at the right and bottom edge stick out)
template <class F> void for_each_local_pixel(const std::vector<int32_t> &blocks, int width, int height, F &&f)
{
	const int blocks_x = (width + kBlockDim - 1) / kBlockDim;
	for(size_t L = 0; L < blocks.size() * kBlockPixels; ++L)
	{
		int x, y;
		block_pixel_xy(blocks[L / kBlockPixels], (int)(L % kBlockPixels), blocks_x, &x, &y);
		if(x < width && y < height) f(L, x, y);
	}
}

}  // namespace adypt
