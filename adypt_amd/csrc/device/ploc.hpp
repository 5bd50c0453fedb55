// A binary tree over the sorted leaves of lbvh.hpp by PLOC, parallel locally-ordered clustering (Meister and Bittner, "Parallel locally-ordered clustering
// for bounding volume hierarchy construction", 2018; Benthin et al., "PLOC++", 2022): THE definition for host (adypt_bvh_build_ploc, adypt_ploc_tree) and
// device (build.hip, adypt_rebuild_bvh_ploc).  No HIP needed (a host compiler may include it), binary32, the operations in the order written, no fma
// and no libm — tests/ploc_truth.py restates the pairing in numpy float32.
//
// Keys, centroid box, sort and node ids are lbvh.hpp's: the leaf of sorted position j is n - 1 + j, the inner nodes are 0 .. n - 2, the root is 0.  What
// changes is the binary tree: instead of Karras's radix tree it is built bottom up, in rounds, and what comes after it (the cut, the layout, the boxes)
// is again what the linear tree uses.
//
// Clusters.  A cluster is a node with its exact box; the list starts as the n leaves in sorted order.
// Distance.  ploc_distance(a, b) = cut_area(refit_union(a, b)); the union does not depend on its order, so d(a, b) and d(b, a) are the same bits.
// One round over m clusters, radius r.  Cluster i scans j = i - r .. i + r in ascending order, without j == i and without anything outside [0, m), and
// keeps the first j whose distance is strictly less than the best so far, which starts at +inf (ploc_nearest; -1: no such j — every distance is +inf
// or NaN).  i and j merge when each is the other's choice.  The cluster at the lower position becomes the new node, with the cluster it was as the LEFT
// child and the other one as the right child; the cluster at the higher position leaves the list; the others keep their order.
// Ids.  A round with k merges takes the k inner ids just below the ones given out so far (the first round's end at n - 2), in ascending order of the
// pair's lower position: the merge of ordinal q takes  next - k + q,  where next starts at n - 1 and drops by k per round.  n - 1 merges happen in all,
// so the last one is node 0: the root.
//
// Progress.  A round over m >= 2 clusters whose distances are all finite merges at least one pair.  Let d be the smallest distance of any pair (i, j)
// with |i - j| <= r, and a the smallest position that is part of a pair at distance d.  Nothing a sees is below d, so a's choice is the first j with
// d(a, j) == d; call it b.  b > a, for b < a would be a smaller position in a pair at d.  Nothing b sees is below d either, so b chooses the first j
// with d(b, j) == d; every such j is part of a pair at d, hence >= a, and a itself is one (the distance is symmetric to the bit and |a - b| <= r both
// ways).  So b chooses a: they merge.  Ties, and 300 copies of one triangle, are therefore no obstacle; a distance that is +inf or NaN is never chosen,
// so a round may then merge nothing — the builders take a round without a merge as the end of the build (ADYPT_E_INVALID), they never repeat it.
// Refusals.  A leaf whose area is not a finite number (a vertex that is NaN, infinite or huge) is refused before the first round.
#pragma once
#include "refit.hpp"
#include "wide_cut.hpp"

namespace adypt {

constexpr int kPlocMinRadius = 1, kPlocMaxRadius = 32, kPlocDefaultRadius = 8;

ADYPT_HOST_DEVICE bool ploc_finite(float v) { return v > -refit_inf() && v < refit_inf(); }

ADYPT_HOST_DEVICE float ploc_distance(const RefitBox &a, const RefitBox &b)
{
	const RefitBox u = refit_union(a, b);
	return cut_area(u.lo, u.hi);
}

// Boxes: RefitBox box(int64_t position) for the positions [max(i - r, 0), min(i + r, m - 1)].  The choice of cluster i of m, or -1.
template <class Boxes> ADYPT_HOST_DEVICE int64_t ploc_nearest(const Boxes &boxes, int64_t m, int64_t i, int r)
{
	const RefitBox me = boxes.box(i);
	const int64_t first = i - r < 0 ? 0 : i - r, last = i + r > m - 1 ? m - 1 : i + r;
	float best = refit_inf();
	int64_t pick = -1;
	for(int64_t j = first; j <= last; ++j)
	{
		if(j == i) continue;
		const float d = ploc_distance(me, boxes.box(j));
		if(d < best) { best = d; pick = j; }
	}
	return pick;
}

// what cluster i does in a round, from everybody's choice
enum PlocRole { kPlocStays = 0, kPlocMerges = 1, kPlocLeaves = 2 }; // kPlocMerges: the lower position of a pair — it becomes the new node
ADYPT_HOST_DEVICE int ploc_role(const int32_t *nearest, int64_t i)
{
	const int64_t j = nearest[i];
	if(j < 0 || (int64_t)nearest[j] != i) return kPlocStays;
	return i < j ? kPlocMerges : kPlocLeaves;
}

// the id of the round's merge of ordinal q of k, when the ids from `next` on are given out
ADYPT_HOST_DEVICE int32_t ploc_merge_id(int64_t next, int64_t k, int64_t q) { return (int32_t)(next - k + q); }

}  // namespace adypt
