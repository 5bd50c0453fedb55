// The binary tree of adypt_bvh_build_linear (include/adypt_host.h): Morton keys, std::sort, Karras's radix tree — the definition is ../device/lbvh.hpp, the
// text the device builder (build.hip) compiles too — laid out as the collapse (wide_builder.cpp) expects a binary tree: pre-order, the right child
// behind its parent, a child's index above its parent's.
#include "builders.hpp"
#include "../device/lbvh.hpp"

#include <algorithm>
#include <chrono>

namespace adypt {

void lbvh_sorted_keys(const TriRec *tris, int64_t n, std::vector<uint64_t> *out)
{
	RefitBox cbox = refit_empty_box();
	for(int64_t i = 0; i < n; ++i)
	{
		float p[9];
		memcpy(p, tris[i].p, sizeof(p));
		for(int k = 0; k < 3; ++k) { const float c = lbvh_centroid(p, k); cbox.lo[k] = refit_min(cbox.lo[k], c); cbox.hi[k] = refit_max(cbox.hi[k], c); }
	}
	std::vector<uint64_t> &keys = *out;
	keys.resize((size_t)n);
	for(int64_t i = 0; i < n; ++i)
	{
		float p[9];
		memcpy(p, tris[i].p, sizeof(p));
		keys[(size_t)i] = lbvh_key(p, cbox, (uint32_t)i);
	}
	std::sort(keys.begin(), keys.end());
}

// a binary tree in the node ids of lbvh.hpp (left, right: n - 1 entries; the root is 0) -> pre-order with exact boxes; the PLOC tree's too (ploc_builder.cpp)
void layout_binary_tree(const TriRec *tris, int64_t n, const std::vector<uint64_t> &keys, const std::vector<int32_t> &left, const std::vector<int32_t> &right, std::vector<BinNode> *bin, int *depth,
                        const RefitBox *ref_box)
{
	// pre-order, right child first
	bin->assign((size_t)(2 * n - 1), BinNode{});
	struct Todo { int32_t id, parent, level; };
	std::vector<Todo> todo{{0, -1, 0}};
	int64_t at = 0;
	int deepest = 0;
	while(!todo.empty())
	{
		const Todo t = todo.back();
		todo.pop_back();
		const int32_t me = (int32_t)at++;
		deepest = std::max(deepest, t.level);
		if(t.parent >= 0) (*bin)[(size_t)t.parent].left = me; // (a right child is parent + 1 and needs no link)
		BinNode &b = (*bin)[(size_t)me];
		if(t.id >= n - 1) // a leaf
		{
			b.tri = (int32_t)(uint32_t)keys[(size_t)(t.id - (n - 1))];
			b.left = -1;
			RefitBox r;
			if(ref_box) r = ref_box[b.tri]; // (b.tri is then the reference: presplit.hpp)
			else
			{
				float p[9];
				memcpy(p, tris[b.tri].p, sizeof(p));
				r = refit_triangle_box(p);
			}
			b.box = Box({r.lo[0], r.lo[1], r.lo[2]}, {r.hi[0], r.hi[1], r.hi[2]});
			continue;
		}
		b.tri = -1;
		todo.push_back({left[(size_t)t.id], me, t.level + 1});
		todo.push_back({right[(size_t)t.id], -1, t.level + 1});
	}
	for(int64_t i = (int64_t)bin->size() - 1; i >= 0; --i)
	{
		BinNode &b = (*bin)[(size_t)i];
		if(b.left == -1) continue;
		const Box &l = (*bin)[(size_t)b.left].box, &r = (*bin)[(size_t)i + 1].box;
		const RefitBox u = refit_union(RefitBox{{l.lo.x, l.lo.y, l.lo.z}, {l.hi.x, l.hi.y, l.hi.z}}, RefitBox{{r.lo.x, r.lo.y, r.lo.z}, {r.hi.x, r.hi.y, r.hi.z}});
		b.box = Box({u.lo[0], u.lo[1], u.lo[2]}, {u.hi[0], u.hi[1], u.hi[2]});
	}
	if(depth) *depth = deepest;
}

int64_t build_lbvh(const TriRec *tris, int64_t n, std::vector<BinNode> *bin, int *depth, double *ms)
{
	const auto t0 = std::chrono::steady_clock::now();
	std::vector<uint64_t> keys;
	lbvh_sorted_keys(tris, n, &keys);
	// the radix tree: node ids as in lbvh.hpp
	std::vector<int32_t> left((size_t)std::max<int64_t>(n - 1, 0)), right(left.size());
	for(int64_t i = 0; i + 1 < n; ++i)
	{
		int64_t first, last, split;
		lbvh_inner_node(keys.data(), n, i, &first, &last, &split);
		left[(size_t)i] = lbvh_left_child(n, first, split);
		right[(size_t)i] = lbvh_right_child(n, last, split);
	}
	layout_binary_tree(tris, n, keys, left, right, bin, depth);
	if(ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return n;
}

}  // namespace adypt
