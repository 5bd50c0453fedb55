// The binary tree of adypt_bvh_build_ploc (include/adypt_host.h): the keys and the sort of the linear BVH, then the rounds of ../device/ploc.hpp — the text
// the device builder (build.hip) compiles too — and the layout of lbvh_builder.cpp for the collapse.  One thread: a round is a few passes over the
// cluster list, and a result that does not depend on the number of threads comes for free.
#include "builders.hpp"
#include "../device/lbvh.hpp"
#include "../device/ploc.hpp"
#include "../device/presplit.hpp"
#include "../../../include/adypt_hip.h"

#include <algorithm>
#include <chrono>

namespace adypt {

namespace {
struct ClusterBoxes {
	const RefitBox *b;
	RefitBox box(int64_t i) const { return b[i]; }
};
}  // namespace

int ploc_tree(const TriRec *tris, int64_t n, int radius, const std::vector<uint64_t> &keys, std::vector<int32_t> *left, std::vector<int32_t> *right, int *rounds, const RefitBox *ref_box)
{
	left->assign((size_t)std::max<int64_t>(n - 1, 0), 0);
	right->assign(left->size(), 0);
	std::vector<int32_t> cluster((size_t)n), nearest((size_t)n);
	std::vector<RefitBox> box((size_t)n);
	for(int64_t j = 0; j < n; ++j)
	{
		if(ref_box) box[(size_t)j] = ref_box[(uint32_t)keys[(size_t)j]];
		else
		{
			float p[9];
			memcpy(p, tris[(uint32_t)keys[(size_t)j]].p, sizeof(p));
			box[(size_t)j] = refit_triangle_box(p);
		}
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

namespace {
// the memory of presplit_walk on the host
struct HostWork {
	RefitBox waiting[kSplitMaxDepth + 1];
	float poly[2][kSplitPolygon][3];
	void put(int depth, const RefitBox &b) { waiting[depth] = b; }
	RefitBox get(int depth) const { return waiting[depth]; }
	float &v(int polygon, int vertex, int axis) { return poly[polygon][vertex][axis]; }
};
struct CountBins {
	float s;
	uint64_t *hist;
	void split(float area) { ++hist[presplit_bin(area, s)]; }
	void leaf(const RefitBox &, int) {}
};
struct CollectLeaves {
	RefitBox *out;
	void split(float) {}
	void leaf(const RefitBox &b, int ordinal) { out[ordinal] = b; }
};
}  // namespace

int presplit_refs(const TriRec *tris, int64_t n, double budget, PresplitRefs *out)
{
	out->level = -1;
	out->n_split = 0;
	out->tri.clear(); out->box.clear(); out->split.clear();
	RefitBox all = refit_empty_box();
	for(int64_t i = 0; i < n; ++i)
	{
		float p[9];
		memcpy(p, tris[i].p, sizeof(p));
		const RefitBox b = refit_triangle_box(p);
		if(!ploc_finite(cut_area(b.lo, b.hi))) { set_host_error("presplit: a triangle whose box has no finite area (vertices that are NaN, infinite or huge)"); return ADYPT_E_INVALID; }
		all = refit_union(all, b);
	}
	int64_t extra = 0;
	float threshold = refit_inf();
	if(budget > 0.0)
	{
		const float s = cut_area(all.lo, all.hi);
		uint64_t roots[kSplitLevels] = {0}, hist[kSplitLevels] = {0};
		HostWork work;
		for(int64_t i = 0; i < n; ++i)
		{
			float p[9];
			memcpy(p, tris[i].p, sizeof(p));
			const int bin = presplit_root_bin(p, s, work);
			if(bin >= 0) ++roots[bin];
		}
		const int64_t allowed = presplit_allowed(budget, n);
		const int top = presplit_level(roots, allowed, &extra); // (no level above this one can be inside the budget: presplit.hpp)
		CountBins count{s, hist};
		for(int64_t i = 0; i < n && top >= 0; ++i)
		{
			float p[9];
			memcpy(p, tris[i].p, sizeof(p));
			presplit_walk(p, presplit_threshold(s, top), work, count);
		}
		out->level = presplit_level(hist, allowed, &extra, top);
		if(out->level >= 0) threshold = presplit_threshold(s, out->level);
	}
	if(n + extra > ((int64_t)1 << 30)) { set_host_error("presplit: more than 2^30 references"); return ADYPT_E_INVALID; }
	out->tri.reserve((size_t)(n + extra)); out->box.reserve((size_t)(n + extra)); out->split.reserve((size_t)(n + extra));
	HostWork work;
	RefitBox leaves[kSplitMaxRefs];
	CollectLeaves collect{leaves};
	for(int64_t i = 0; i < n; ++i)
	{
		float p[9];
		memcpy(p, tris[i].p, sizeof(p));
		const int k = extra > 0 ? presplit_walk(p, threshold, work, collect) : 1;
		if(k == 1) leaves[0] = refit_triangle_box(p);
		else ++out->n_split;
		for(int q = 0; q < k; ++q) { out->tri.push_back((int32_t)i); out->box.push_back(leaves[q]); out->split.push_back(k > 1); }
	}
	if((int64_t)out->tri.size() != n + extra) { set_host_error("presplit: the references do not add up to the counted ones"); return ADYPT_E_INVALID; }
	return ADYPT_OK;
}

static void presplit_sorted_keys(const TriRec *tris, const PresplitRefs &refs, std::vector<uint64_t> *out)
{
	const int64_t n = (int64_t)refs.tri.size();
	std::vector<float> centroid((size_t)n * 3);
	RefitBox cbox = refit_empty_box();
	for(int64_t r = 0; r < n; ++r)
	{
		float p[9];
		memcpy(p, tris[refs.tri[(size_t)r]].p, sizeof(p));
		for(int k = 0; k < 3; ++k)
		{
			const float c = refs.split[(size_t)r] ? presplit_centroid(refs.box[(size_t)r], k) : lbvh_centroid(p, k);
			centroid[(size_t)r * 3 + k] = c;
			cbox.lo[k] = refit_min(cbox.lo[k], c); cbox.hi[k] = refit_max(cbox.hi[k], c);
		}
	}
	out->resize((size_t)n);
	for(int64_t r = 0; r < n; ++r) (*out)[(size_t)r] = lbvh_key_of(&centroid[(size_t)r * 3], cbox, (uint32_t)r);
	std::sort(out->begin(), out->end());
}

int64_t build_ploc_split(const TriRec *tris, int64_t n, int radius, const PresplitRefs &refs, std::vector<BinNode> *bin, int *depth, double *ms)
{
	const auto t0 = std::chrono::steady_clock::now();
	const int64_t n_refs = (int64_t)refs.tri.size();
	std::vector<uint64_t> keys;
	presplit_sorted_keys(tris, refs, &keys);
	std::vector<int32_t> left, right;
	if(ploc_tree(tris, n_refs, radius, keys, &left, &right, nullptr, refs.box.data()) != ADYPT_OK) return -1;
	layout_binary_tree(tris, n_refs, keys, left, right, bin, depth, refs.box.data());
	if(ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return n_refs;
}

}  // namespace adypt
