// Internal interface of the CPU BVH producers (binary SBVH -> 8-wide compressed BVH).
#pragma once
#include "common.hpp"
#include "../../../include/adypt_host.h"

namespace adypt {

// returns the number of leaves (= triangle references incl. spatial-split duplicates); the node array does not
// depend on n_threads
int64_t build_sbvh(const TriRec *tris, int64_t n_tris, const Box &scene_box, const adypt_bvh_params &cfg,
				   std::vector<BinNode> *nodes, double *ms, int n_threads);

// the binary tree of a linear BVH (../device/lbvh.hpp) in the layout build_wide_bvh expects: one leaf per triangle, no splits.  *depth: the edges of
// the longest path from the root to a leaf.  Returns the number of leaves.
void lbvh_sorted_keys(const TriRec *tris, int64_t n_tris, std::vector<uint64_t> *keys); // Morton code << 32 | triangle index, ascending
int64_t build_lbvh(const TriRec *tris, int64_t n_tris, std::vector<BinNode> *nodes, int *depth, double *ms);

void build_wide_bvh(const std::vector<BinNode> &bin, int64_t leaf_count, const adypt_bvh_params &cfg,
					std::vector<NodeRec> *nodes, std::vector<int32_t> *tri_indices, double *ms, int n_threads);

}  // namespace adypt
