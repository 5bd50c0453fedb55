// Adaptive sampling: which owned 32x32 blocks a pass still traces.  An owned block is ACTIVE (it advances with the context's frame counter) or
// FROZEN at spp_b (it reached the noise target after spp_b frames and holds, bit for bit, the pixels of the uniform image at spp_b).  Here: the
// state, the freeze decision, and what adypt_trace_adaptive and adypt_multi_trace_adaptive do after each step of THE loop (trace_until.hpp).  No HIP
// and no adypt_ctx (a host compiler may include it: tests/test_active_blocks.py steps the loop over scripted block noise).
//
// The persistent images (accum, the noise moments, everything the read-outs and the gathers touch) stay in owned-block order whatever is
// frozen.  A pass over a shrunken set runs the same kernels on a shorter list: SceneArgs::local_blocks = `active`, FrameArgs::n_local_px =
// active.size() x 1024; done[] and the ray queues are indexed by that pass-local pixel, and the running-mean kernel maps pass-local pixel P to
// owned pixel slot[P >> 10] * 1024 + (P & 1023).
#pragma once
#include "tile_layout.hpp"
#include "noise.hpp"
#include "trace_until.hpp"
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

// The freeze decision: worst_block's comparison (noise.hpp noise_of_image: sum / count in binary64 against the target), taken per block.  A block
// without a pixel inside the image has nothing left to sample.
inline bool block_converged(double sum, uint32_t count, double target) { return count == 0 || sum / (double)count <= target; }

// What the call reports from the blocks of its last check (ascending block index; each at its own sample count)
inline adypt_adaptive adaptive_result(const std::vector<BlockState> &blocks, int counter)
{
	adypt_adaptive a;
	memset(&a, 0, sizeof(a));
	for(const BlockState &b : blocks)
	{
		a.noise.pixels += b.count;
		a.pixel_samples += (int64_t)b.count * (int64_t)b.spp;
		a.blocks_frozen += b.frozen ? 1 : 0;
	}
	a.blocks = (int32_t)blocks.size();
	const NoiseImage img = noise_of_image(blocks.data(), blocks.size(), a.noise.pixels);
	a.noise.mean_noise = img.mean_noise; a.noise.worst_block = img.worst_block; a.noise.worst_index = img.worst_index;
	a.noise.spp = counter;
	return a;
}

// spp(): the frame counter; trace(n): n more frames of the active blocks; read_blocks(std::vector<BlockState> *): every block (of the image for
// several devices), ascending block index, each at its own sample count; freeze(blocks, spp): those image blocks stop at spp frames.  The three
// return ADYPT_OK or the code this returns.  THE loop of trace_until.hpp (step_until: its steps, its argument check, nothing read below 2 spp); after
// every step the blocks are read and, from min_spp on, every active one at or below the target is frozen.  The run is over when no block is active; a
// caller without a block (a process-per-GPU rank that owns none) runs to max_spp, as the slowest of its peers may.
template <class Spp, class Trace, class ReadBlocks, class Freeze>
int trace_adaptive(const char *fn, std::string *error, double target, int min_spp, int max_spp, int check_every, adypt_adaptive *out, Spp spp, Trace trace,
                   ReadBlocks read_blocks, Freeze freeze)
{
	std::vector<BlockState> blocks;
	const int r = step_until(fn, error, target, min_spp, max_spp, check_every, spp, trace, [&](int now, bool *finished) {
		const int rc = read_blocks(&blocks);
		if(rc != ADYPT_OK) return rc;
		std::vector<int32_t> stop;
		*finished = !blocks.empty();
		for(BlockState &b : blocks)
		{
			if(!b.frozen && now >= min_spp && block_converged(b.sum, b.count, target)) { b.frozen = true; b.spp = now; stop.push_back(b.index); }
			if(!b.frozen) *finished = false;
		}
		return stop.empty() ? (int)ADYPT_OK : freeze(stop, now);
	});
	if(r != ADYPT_OK) return r;
	if(out) *out = adaptive_result(blocks, spp());
	return ADYPT_OK;
}

}  // namespace adypt
