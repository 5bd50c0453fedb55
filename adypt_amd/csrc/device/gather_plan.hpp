// The one exchange of the sharded frame, decided once: what every rank's compact buffer holds, where it lands on the root, and which sends and
// receives THIS process posts between ncclGroupStart and ncclGroupEnd.  No HIP and no adypt_ctx (a host compiler may include it:
// tests/test_gather_plan.py does); multi.hip executes the plan for a process that owns every rank (adypt_multi) and for one that owns a single
// rank (adypt_comm_*) alike — they differ only in which ranks are local.
#pragma once
#include "tile_layout.hpp"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace adypt {

struct GatherOp {
	enum Kind { Send, Recv } kind;
	int rank;         // Send: the local rank that sends to the root; Recv: the peer the root receives from
	int64_t elements; // floats: 4 x the rank's float4 count
	int64_t offset;   // float4 into the root's gather buffer (Send: where the data will land)
};

struct GatherPlan {
	std::vector<int64_t> counts; // float4 elements of rank r's compact block-major buffer (every rank computes the same)
	int64_t stride = 0;          // rank r's tiles land at gathered + r * stride; the buffer is stride x nranks float4
	std::vector<GatherOp> ops;   // in posting order
};

// `local`: the ranks this process owns.  Peer by peer, ascending, a peer that owns no block skipped: its send if the peer is local, then the
// root's receive if the root is local.
inline GatherPlan plan_gather(int width, int height, int nranks, const std::vector<int> &local)
{
	GatherPlan p;
	std::vector<char> is_local((size_t)nranks, 0);
	for(int r : local)
		if(r >= 0 && r < nranks) is_local[(size_t)r] = 1;
	for(int r = 0; r < nranks; ++r) p.counts.push_back((int64_t)owned_blocks(width, height, r, nranks).size() * kBlockPixels);
	p.stride = 1024;
	for(int64_t c : p.counts) p.stride = std::max(p.stride, c);
	for(int r = 1; r < nranks; ++r)
	{
		const int64_t c = p.counts[(size_t)r];
		if(c == 0) continue;
		if(is_local[(size_t)r]) p.ops.push_back({GatherOp::Send, r, 4 * c, r * p.stride});
		if(is_local[0]) p.ops.push_back({GatherOp::Recv, r, 4 * c, r * p.stride});
	}
	return p;
}

}  // namespace adypt
