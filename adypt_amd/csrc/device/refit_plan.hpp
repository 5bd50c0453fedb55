// The order in which a refit visits the nodes of a CWBVH8, decided once per tree: every node's depth by a walk from the root (node 0) and the nodes
// of every level.  A level's nodes depend only on deeper levels, so refitting level by level, deepest first, is the whole dependency: the host loops
// (adypt_bvh_refit), the device launches k_refit_nodes once per level on one stream (refit.hip).  No HIP and no adypt_ctx: a host compiler may include it
// (tests/test_refit_definition.py does).
//
// The walk is also the validation.  It refuses, with a reason and without reading out of range: a child index or a reference range outside the arrays,
// a leaf whose top bits are none of 001 / 011 / 111, a node reached twice (a shared child or a cycle) and a node never reached.
#pragma once
#include "refit.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace adypt {

struct RefitPlan {
	std::vector<int32_t> depth;        // per node; the root's is 0
	std::vector<int32_t> order;        // the nodes level by level, the root's level first, ascending node index inside a level
	std::vector<int64_t> level_begin;  // level l is order[level_begin[l] .. level_begin[l + 1]); levels() + 1 entries
	int levels() const { return (int)level_begin.size() - 1; }
};

// nodes: n_nodes records of 80 bytes.  false: *why says which node and what; *plan is then unspecified.
inline bool plan_refit(const void *nodes_, int64_t n_nodes, int64_t n_refs, RefitPlan *plan, std::string *why)
{
	const uint8_t *nodes = (const uint8_t *)nodes_;
	if(!nodes || n_nodes <= 0 || n_nodes > INT32_MAX || n_refs < 0) { *why = "empty or oversized node array"; return false; }
	plan->depth.assign((size_t)n_nodes, -1);
	plan->depth[0] = 0;
	std::vector<int32_t> level(1, 0), next;
	std::vector<std::vector<int32_t>> levels;
	int64_t reached = 0;
	while(!level.empty())
	{
		next.clear();
		for(int32_t i : level)
		{
			const uint8_t *n = nodes + (size_t)i * kNodeBytes;
			uint32_t child_base, tri_base;
			memcpy(&child_base, n + kNodeChildBase, 4);
			memcpy(&tri_base, n + kNodeTriBase, 4);
			for(int s = 0; s < 8; ++s)
			{
				const uint32_t meta = n[kNodeMeta + s];
				const int kind = refit_slot_kind(meta);
				if(kind == kSlotInternal)
				{
					const uint64_t child = (uint64_t)child_base + refit_child_offset(meta);
					if(child >= (uint64_t)n_nodes) { *why = "node " + std::to_string(i) + ": child index out of range"; return false; }
					if(plan->depth[(size_t)child] != -1) { *why = "node " + std::to_string(child) + " is reached twice"; return false; }
					plan->depth[(size_t)child] = (int32_t)levels.size() + 1;
					next.push_back((int32_t)child);
				}
				else if(kind == kSlotLeaf)
				{
					const int count = refit_leaf_count(meta);
					if(count == 0) { *why = "node " + std::to_string(i) + ": leaf bits are none of 001, 011, 111"; return false; }
					if((uint64_t)tri_base + refit_leaf_offset(meta) + (uint64_t)count > (uint64_t)n_refs) { *why = "node " + std::to_string(i) + ": reference range out of range"; return false; }
				}
			}
		}
		reached += (int64_t)level.size();
		levels.push_back(level);
		level.swap(next);
	}
	if(reached != n_nodes) { *why = std::to_string(n_nodes - reached) + " node(s) are not reached from the root"; return false; }
	plan->order.clear();
	plan->level_begin.assign(1, 0);
	for(std::vector<int32_t> &l : levels)
	{
		std::sort(l.begin(), l.end());
		plan->order.insert(plan->order.end(), l.begin(), l.end());
		plan->level_begin.push_back((int64_t)plan->order.size());
	}
	return true;
}

}  // namespace adypt
