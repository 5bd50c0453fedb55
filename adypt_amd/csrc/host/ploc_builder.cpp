// The binary tree of adypt_bvh_build_ploc (include/adypt_host.h): the keys and the sort of the linear BVH, then the rounds of ../device/ploc.hpp — the text
// the device builder (build.hip) compiles too — and the layout of lbvh_builder.cpp for the collapse.  One thread: a round is a few passes over the
// cluster list, and a result that does not depend on the number of threads comes for free.
#include "builders.hpp"
#include "../device/ploc.hpp"
#include "../../../include/adypt_hip.h"

#include <chrono>

namespace adypt {

namespace {
struct ClusterBoxes {
	const RefitBox *b;
	RefitBox box(int64_t i) const { return b[i]; }
};
}  // namespace

int ploc_tree(const TriRec *tris, int64_t n, int radius, const std::vector<uint64_t> &keys, std::vector<int32_t> *left, std::vector<int32_t> *right, int *rounds)
{
	left->assign((size_t)std::max<int64_t>(n - 1, 0), 0);
	right->assign(left->size(), 0);
	std::vector<int32_t> cluster((size_t)n), nearest((size_t)n);
	std::vector<RefitBox> box((size_t)n);
	for(int64_t j = 0; j < n; ++j)
	{
		float p[9];
		memcpy(p, tris[(uint32_t)keys[(size_t)j]].p, sizeof(p));
		box[(size_t)j] = refit_triangle_box(p);
		cluster[(size_t)j] = (int32_t)(n - 1 + j);
		if(!ploc_finite(cut_area(box[(size_t)j].lo, box[(size_t)j].hi))) { set_host_error("ploc: a triangle whose box has no finite area (vertices that are NaN, infinite or huge)"); return ADYPT_E_INVALID; }
	}
	int n_rounds = 0;
	for(int64_t m = n, next = n - 1; m > 1; ++n_rounds)
	{
		const ClusterBoxes boxes{box.data()};
		for(int64_t i = 0; i < m; ++i) nearest[(size_t)i] = (int32_t)ploc_nearest(boxes, m, i, radius);
		int64_t k = 0;
		for(int64_t i = 0; i < m; ++i) k += ploc_role(nearest.data(), i) == kPlocMerges;
		if(k == 0) { set_host_error("ploc: a round merged nothing (distances that are infinite or NaN)"); return ADYPT_E_INVALID; }
		// in place: a cluster's new position `at` is never above its old one i, and everything read from here on lies at i or above
		int64_t at = 0, q = 0;
		for(int64_t i = 0; i < m; ++i)
		{
			const int role = ploc_role(nearest.data(), i);
			if(role == kPlocLeaves) continue;
			int32_t id = cluster[(size_t)i];
			RefitBox b = box[(size_t)i];
			if(role == kPlocMerges)
			{
				const int64_t j = nearest[(size_t)i];
				id = ploc_merge_id(next, k, q++);
				(*left)[(size_t)id] = cluster[(size_t)i];
				(*right)[(size_t)id] = cluster[(size_t)j];
				b = refit_union(b, box[(size_t)j]);
			}
			cluster[(size_t)at] = id;
			box[(size_t)at] = b;
			++at;
		}
		next -= k;
		m = at;
	}
	if(rounds) *rounds = n_rounds;
	return ADYPT_OK;
}

int64_t build_ploc(const TriRec *tris, int64_t n, int radius, std::vector<BinNode> *bin, int *depth, double *ms)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<uint64_t> keys;
	lbvh_sorted_keys(tris, n, &keys);
	std::vector<int32_t> left, right;
	if(ploc_tree(tris, n, radius, keys, &left, &right, nullptr) != ADYPT_OK) return -1;
	layout_binary_tree(tris, n, keys, left, right, bin, depth);
	if(ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return n;
}

}  // namespace adypt
