// Internal interface of the CPU BVH producers (binary SBVH -> 8-wide compressed BVH).
#pragma once
#include "common.hpp"
#include "../device/refit.hpp"
#include "../../../include/adypt_host.h"

namespace adypt {

// returns the number of leaves (= triangle references incl. spatial-split duplicates); the node array does not
// depend on n_threads.  -1: a node for which no split costs less than FLT_MAX (areas that overflow, or are NaN) — the build would not end
int64_t build_sbvh(const TriRec *tris, int64_t n_tris, const Box &scene_box, const adypt_bvh_params &cfg,
				   std::vector<BinNode> *nodes, double *ms, int n_threads);

// the binary tree of a linear BVH (../device/lbvh.hpp) in the layout build_wide_bvh expects: one leaf per triangle, no splits.  *depth: the edges of
// the longest path from the root to a leaf.  Returns the number of leaves.
void lbvh_sorted_keys(const TriRec *tris, int64_t n_tris, std::vector<uint64_t> *keys); // Morton code << 32 | triangle index, ascending
int64_t build_lbvh(const TriRec *tris, int64_t n_tris, std::vector<BinNode> *nodes, int *depth, double *ms);
// left, right: the children of the inner nodes 0 .. n - 2 in the node ids of lbvh.hpp (leaf of sorted position j: n - 1 + j)
void layout_binary_tree(const TriRec *tris, int64_t n_tris, const std::vector<uint64_t> &keys, const std::vector<int32_t> &left, const std::vector<int32_t> &right, std::vector<BinNode> *nodes,
                        int *depth, const RefitBox *ref_box = nullptr); // ref_box: the leaves are references (the keys' low words), these their boxes

// the binary tree of ../device/ploc.hpp over the sorted keys, in the node ids of lbvh.hpp.  *rounds: the rounds it took.  ADYPT_E_INVALID for a leaf
// whose area is no finite number and for a round that merges nothing; sequential, so the same for any number of threads
int ploc_tree(const TriRec *tris, int64_t n_tris, int radius, const std::vector<uint64_t> &keys, std::vector<int32_t> *left, std::vector<int32_t> *right, int *rounds,
              const RefitBox *ref_box = nullptr);
// ... laid out as build_lbvh lays out its tree.  Returns the number of leaves, or -1 where ploc_tree refuses
int64_t build_ploc(const TriRec *tris, int64_t n_tris, int radius, std::vector<BinNode> *nodes, int *depth, double *ms);

// the references of ../device/presplit.hpp: triangles split into several, each with its box.  level: the chosen one, or -1; n_split: triangles with more
// than one reference; split[r]: reference r is one of several.  ADYPT_E_INVALID for a triangle whose box has no finite area.  Sequential.
struct PresplitRefs { int level = -1; int64_t n_split = 0; std::vector<int32_t> tri; std::vector<RefitBox> box; std::vector<uint8_t> split; };
int presplit_refs(const TriRec *tris, int64_t n_tris, double budget, PresplitRefs *out);
// build_ploc over those references: a leaf's `tri` is its reference.  Returns the number of leaves, or -1 where ploc_tree refuses
int64_t build_ploc_split(const TriRec *tris, int64_t n_tris, int radius, const PresplitRefs &refs, std::vector<BinNode> *nodes, int *depth, double *ms);
// adypt_bvh_refit with the box of every reference given (ref_boxes, in the order of tri_indices) instead of its whole triangle's; nullptr: adypt_bvh_refit
int bvh_refit_boxes(void *nodes, int64_t n_nodes, const int32_t *tri_indices, int64_t n_refs, const void *triangles, int64_t n_tris, const RefitBox *ref_boxes);

// false: the SAH costs of some node are not finite numbers below FLT_MAX (../device/wide_cut.hpp cut_inner_row); the arrays are then empty
bool build_wide_bvh(const std::vector<BinNode> &bin, int64_t leaf_count, const adypt_bvh_params &cfg,
					std::vector<NodeRec> *nodes, std::vector<int32_t> *tri_indices, double *ms, int n_threads);

}  // namespace adypt
