// Adaptive sampling: which owned 32x32 blocks a pass still traces.  An owned block is ACTIVE (it advances with the context's frame counter) or
// FROZEN at spp_b (it reached the noise target after spp_b frames and holds, bit for bit, the pixels of the uniform image at spp_b).  Here: the
// state, the freeze decision, and THE loop of adypt_trace_adaptive and adypt_multi_trace_adaptive over whatever traces.  No HIP and no adypt_ctx
// (a host compiler may include it: tests/test_active_blocks.py steps the loop over scripted block noise).
//
// The persistent images (accum, the noise moments, everything the read-outs and the gathers touch) stay in owned-block order whatever is
// frozen.  A pass over a shrunken set runs the same kernels on a shorter list: SceneArgs::local_blocks = `active`, FrameArgs::n_local_px =
// active.size() x 1024; done[] and the ray queues are indexed by that pass-local pixel, and the running-mean kernel maps pass-local pixel P to
// owned pixel slot[P >> 10] * 1024 + (P & 1023).
#pragma once
#include "tile_layout.hpp"
#include "noise.hpp"
#include "../../../include/adypt_hip.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace adypt {

struct ActiveBlocks {
	std::vector<int32_t> owned;     // image block index of every owned block, ascending (tile_layout.hpp owned_blocks)
	std::vector<int32_t> frozen_at; // per owned block: 0 = active, else spp_b (>= 2: nothing freezes before it has a variance estimate)
	std::vector<int32_t> active;    // image block index of the active blocks, ascending: a subsequence of `owned`
	std::vector<int32_t> slot;      // per active block: its place in `owned`
	int n_frozen = 0;

	void reset(const std::vector<int32_t> &owned_list) { owned = owned_list; thaw(); }
	// everything active again: active == owned, slot == 0, 1, 2, ...
	void thaw()
	{
		frozen_at.assign(owned.size(), 0);
		n_frozen = 0;
		rebuild();
	}
	bool any_frozen() const { return n_frozen > 0; }
	// image block `block` is this list's and active
	bool is_active(int32_t block) const
	{
		const auto it = std::lower_bound(owned.begin(), owned.end(), block);
		return it != owned.end() && *it == block && frozen_at[(size_t)(it - owned.begin())] == 0;
	}
	// frames in owned block i when the context's counter is at `counter`
	int spp_of(size_t i, int counter) const { return frozen_at[i] ? frozen_at[i] : counter; }
	// Freezes the owned blocks among `blocks` (image block indices, any order; blocks of other owners and blocks already frozen are passed over)
	// at `spp` >= 2 frames (fewer: nothing changes).  Returns how many changed state; the active list and the slot map are current afterwards.
	int freeze(const std::vector<int32_t> &blocks, int spp)
	{
		int changed = 0;
		for(int32_t b : blocks)
		{
			const auto it = std::lower_bound(owned.begin(), owned.end(), b);
			if(it == owned.end() || *it != b) continue;
			int32_t &at = frozen_at[(size_t)(it - owned.begin())];
			if(at == 0 && spp >= 2) { at = spp; ++changed; }
		}
		if(changed) { n_frozen += changed; rebuild(); }
		return changed;
	}
	// pixels of the active blocks that lie inside the image (= camera rays per frame of a pass)
	int64_t active_image_px(int width, int height) const
	{
		const int blocks_x = (width + kBlockDim - 1) / kBlockDim;
		int64_t n = 0;
		for(int32_t b : active)
			n += (int64_t)std::min(kBlockDim, width - (b % blocks_x) * kBlockDim) * (int64_t)std::min(kBlockDim, height - (b / blocks_x) * kBlockDim);
		return n;
	}

private:
	void rebuild()
	{
		active.clear(); slot.clear();
		for(size_t i = 0; i < owned.size(); ++i)
			if(frozen_at[i] == 0) { active.push_back(owned[i]); slot.push_back((int32_t)i); }
	}
};

// one block as the loop sees it: adypt_read_block_noise's (index, sum, count), the frames it holds and whether it is frozen at them
struct BlockState { int32_t index; double sum; uint32_t count; int32_t spp; bool frozen; };

// The freeze decision: worst_block's comparison (noise.hpp noise_of_image: sum / count in binary64 against the target), taken per block.  A block
// without a pixel inside the image has nothing left to sample.
inline bool block_converged(double sum, uint32_t count, double target) { return count == 0 || sum / (double)count <= target; }

// What the call reports from the blocks of its last check (ascending block index; each at its own sample count)
inline adypt_adaptive adaptive_result(const std::vector<BlockState> &blocks, int counter)
{
	adypt_adaptive a;
	memset(&a, 0, sizeof(a));
	std::vector<int32_t> index;
	std::vector<double> sum;
	std::vector<uint32_t> count;
	for(const BlockState &b : blocks)
	{
		index.push_back(b.index); sum.push_back(b.sum); count.push_back(b.count);
		a.noise.pixels += b.count;
		a.pixel_samples += (int64_t)b.count * (int64_t)b.spp;
		a.blocks_frozen += b.frozen ? 1 : 0;
	}
	a.blocks = (int32_t)blocks.size();
	const NoiseImage img = noise_of_image(index.data(), sum.data(), count.data(), blocks.size(), a.noise.pixels);
	a.noise.mean_noise = img.mean_noise; a.noise.worst_block = img.worst_block; a.noise.worst_index = img.worst_index;
	a.noise.spp = counter;
	return a;
}

// spp(): the frame counter; trace(n): n more frames of the active blocks; read_blocks(std::vector<BlockState> *): every block (of the image for
// several devices), ascending block index, each at its own sample count (asked only at 2 spp and more); freeze(blocks, spp): those image blocks
// stop at spp frames.  The three return ADYPT_OK or the code this returns.  Steps of check_every, the last one cut to reach max_spp exactly, as
// trace_until.hpp; after every step the blocks are read and, from min_spp on, every active one at or below the target is frozen.  The loop ends when
// no block is active or at max_spp; a caller without a block (a process-per-GPU rank that owns none) runs to max_spp, as the slowest of its peers
// may.  `fn` names the caller in *error, which is written only when the arguments are refused (nothing is traced then).
template <class Spp, class Trace, class ReadBlocks, class Freeze>
int trace_adaptive(const char *fn, std::string *error, double target, int min_spp, int max_spp, int check_every, adypt_adaptive *out, Spp spp, Trace trace,
                   ReadBlocks read_blocks, Freeze freeze)
{
	if(check_every < 1 || min_spp < 2 || max_spp < min_spp || !(target == target))
	{
		*error = std::string(fn) + ": needs check_every >= 1, 2 <= min_spp <= max_spp and a target that is a number";
		return ADYPT_E_INVALID;
	}
	std::vector<BlockState> blocks;
	for(;;)
	{
		const int n = std::min(check_every, max_spp - spp());
		int r = n > 0 ? trace(n) : ADYPT_OK;
		if(r != ADYPT_OK) return r;
		const int now = spp();
		bool none_active = false;
		if(now >= 2)
		{
			if((r = read_blocks(&blocks)) != ADYPT_OK) return r;
			std::vector<int32_t> stop;
			none_active = !blocks.empty();
			for(BlockState &b : blocks)
			{
				if(!b.frozen && now >= min_spp && block_converged(b.sum, b.count, target)) { b.frozen = true; b.spp = now; stop.push_back(b.index); }
				if(!b.frozen) none_active = false;
			}
			if(!stop.empty() && (r = freeze(stop, now)) != ADYPT_OK) return r;
		}
		if(n <= 0 || now >= max_spp || none_active) break;
	}
	if(out) *out = adaptive_result(blocks, spp());
	return ADYPT_OK;
}

}  // namespace adypt
