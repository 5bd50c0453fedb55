// A CWBVH8 from the triangles alone, by a linear BVH: THE definition for host (adypt_bvh_build_linear) and device (build.hip, adypt_rebuild_bvh).  No HIP
// needed (a host compiler may include it), binary32, the operations in the order written, no fma and no libm — tests/lbvh_truth.py restates the keys
// in numpy float32.
//
// Keys.  A triangle's centroid is ((p0 + p1) + p2) * float(1 / 3) per axis; the centroid box is taken with refit_min / refit_max (refit.hpp), so it does
// not depend on the order it is taken in.  Per axis the 10-bit cell is (c - lo) * (1024 / (hi - lo)) cut off to an integer, at most 1023, and 0 for
// anything that is not a positive finite number (a zero extent gives 0 * inf = NaN, hence 0).  The three cells are interleaved, x highest, to a 30-bit
// Morton code; the sort key is code << 32 | triangle index.  Keys are unique: the sorted order is a function of the triangles alone and any correct
// sort gives it.
//
// The binary tree is Karras's radix tree over the sorted keys ("Maximizing parallelism in the construction of BVHs, octrees and k-d trees", 2012), delta
// = the length of the common prefix of two 64-bit keys.  n keys give n - 1 inner nodes; here a node is one int: inner node i is i, the leaf of sorted
// position j is n - 1 + j, and the root is 0 (also for n = 1, where it is the only leaf).  A node's exact box is the union of its triangles'
// refit_triangle_box; the number of triangles goes up with it.
//
// The cut is wide_cut.hpp's, unchanged.  The layout is the collapse's (host/wide_builder.cpp): a wide node, given where its children and its references
// start, takes the next nodes for its inner children in slot order and the next references for its leaf slots in slot order; then every inner child, in
// gather order, gets the run behind that: wide_below - 1 nodes and tri_count references.  So positions follow top down from counts taken bottom up, and
// no allocation order shows in the result.  lbvh_emit_node writes the topology of one node (child_base, tri_base, meta, imask; the box bytes zero) and
// names its inner children with their runs; the boxes are then the refit's (refit.hpp), on both sides.
#pragma once
#include "refit.hpp"
#include "wide_cut.hpp"

namespace adypt {

// p: 9 floats, the three vertices
ADYPT_HOST_DEVICE float lbvh_centroid(const float *p, int k) { return ((p[k] + p[3 + k]) + p[6 + k]) * float(1.0 / 3); }

ADYPT_HOST_DEVICE uint32_t lbvh_cell(float c, float lo, float hi)
{
	const float q = (c - lo) * (1024.0f / (hi - lo));
	if(!(q > 0.0f && q < refit_inf())) return 0u;
	return q < 1023.0f ? (uint32_t)(int)q : 1023u;
}
// 10 bits -> every third bit of 30
ADYPT_HOST_DEVICE uint32_t lbvh_spread(uint32_t v)
{
	v = (v | (v << 16)) & 0x030000ffu;
	v = (v | (v << 8)) & 0x0300f00fu;
	v = (v | (v << 4)) & 0x030c30c3u;
	v = (v | (v << 2)) & 0x09249249u;
	return v;
}
// c: a centroid; box: the centroid box
ADYPT_HOST_DEVICE uint64_t lbvh_key_of(const float *c, const RefitBox &box, uint32_t index)
{
	uint32_t cell[3];
	for(int k = 0; k < 3; ++k) cell[k] = lbvh_cell(c[k], box.lo[k], box.hi[k]);
	const uint32_t code = lbvh_spread(cell[0]) << 2 | lbvh_spread(cell[1]) << 1 | lbvh_spread(cell[2]);
	return (uint64_t)code << 32 | index;
}
ADYPT_HOST_DEVICE uint64_t lbvh_key(const float *p, const RefitBox &box, uint32_t index)
{
	const float c[3] = {lbvh_centroid(p, 0), lbvh_centroid(p, 1), lbvh_centroid(p, 2)};
	return lbvh_key_of(c, box, index);
}

ADYPT_HOST_DEVICE int lbvh_delta(const uint64_t *keys, int64_t n, int64_t i, int64_t j)
{
	if(j < 0 || j >= n) return -1;
	return __builtin_clzll(keys[i] ^ keys[j]); // (unique keys: never 0 ^ 0)
}
// inner node i of the radix tree over n >= 2 sorted keys: the sorted positions [*first, *last] it covers; its children cover [*first, *split] and
// [*split + 1, *last]
ADYPT_HOST_DEVICE void lbvh_inner_node(const uint64_t *keys, int64_t n, int64_t i, int64_t *first, int64_t *last, int64_t *split)
{
	const int64_t d = lbvh_delta(keys, n, i, i + 1) > lbvh_delta(keys, n, i, i - 1) ? 1 : -1;
	const int dmin = lbvh_delta(keys, n, i, i - d);
	int64_t lmax = 2;
	while(lbvh_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
	int64_t l = 0;
	for(int64_t t = lmax / 2; t >= 1; t /= 2)
		if(lbvh_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
	const int64_t j = i + l * d;
	const int dnode = lbvh_delta(keys, n, i, j);
	int64_t s = 0, t = l;
	do
	{
		t = (t + 1) / 2;
		if(lbvh_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
	} while(t > 1);
	*split = i + s * d + (d < 0 ? -1 : 0);
	*first = d > 0 ? i : j;
	*last = d > 0 ? j : i;
}
// the node ids of the children of an inner node that covers [first, last] and splits behind `split`
ADYPT_HOST_DEVICE int32_t lbvh_left_child(int64_t n, int64_t first, int64_t split) { return (int32_t)(split == first ? n - 1 + split : split); }
ADYPT_HOST_DEVICE int32_t lbvh_right_child(int64_t n, int64_t last, int64_t split) { return (int32_t)(split + 1 == last ? n - 1 + split + 1 : split + 1); }

// a wide node to be emitted: node w is binary node s; its inner children go to node_base .., its references to tri_base ..
struct WideItem { int32_t w, s; uint32_t node_base, tri_base; };

// Tree: wide_cut.hpp's, and   bool is_leaf(int n), int32_t tri(int leaf), int tri_count(int n), void box(int n, float lo[3], float hi[3]).
// rec: the node's 80 bytes as 20 words; tri_indices: the whole reference array of ref_limit entries (nothing is written beyond: counts that disagree
// must not turn into a stray store); kids: the inner children in gather order.  Returns their number.  Placed:  void operator()(const Tree &, uint32_t
// position, int leaf)  is told which binary leaf went to which position of tri_indices (a tree with several references per triangle: presplit.hpp).
struct LbvhNobody { template <class Tree> ADYPT_HOST_DEVICE void operator()(const Tree &, uint32_t, int) const {} };
template <class Tree, class Placed> ADYPT_HOST_DEVICE int lbvh_emit_node(const Tree &t, const WideItem &it, uint32_t rec[20], int32_t *tri_indices, uint32_t ref_limit, WideItem kids[8], const Placed &placed)
{
	int child[8], n_child = 0;
	if(t.is_leaf(it.s)) child[n_child++] = it.s; // the one-triangle scene: the root gets that leaf as its only child
	else cut_gather_children(t, it.s, 1, &n_child, child);
	int slot_of[8];
	{
		float m[8][8], lo[3], hi[3], pc[3];
		t.box(it.s, lo, hi);
		for(int a = 0; a < 3; ++a) pc[a] = (lo[a] + hi[a]) * 0.5f;
		for(int i = 0; i < n_child; ++i)
		{
			float d[3];
			t.box(child[i], lo, hi);
			for(int a = 0; a < 3; ++a) d[a] = (lo[a] + hi[a]) * 0.5f - pc[a];
			for(int j = 0; j < 8; ++j) m[i][j] = cut_slot_cost(d, j);
		}
		cut_assign_slots(m, n_child, slot_of);
	}
	int in_slot[8], widx_of[8];
	for(int i = 0; i < 8; ++i) in_slot[i] = -1;
	for(int i = 0; i < n_child; ++i) in_slot[slot_of[i]] = i;
	for(int k = 0; k < 20; ++k) rec[k] = 0u;
	uint32_t node_at = it.node_base, tri_at = it.tri_base, imask = 0, meta[8];
	for(int i = 0; i < 8; ++i)
	{
		meta[i] = 0;
		if(in_slot[i] < 0) continue;
		const int c = child[in_slot[i]];
		if(t.row(c)[1].type == kLeaf)
		{
			const uint32_t off = tri_at - it.tri_base;
			// right subtree first (a leaf cut holds at most 3 references)
			int cnt = 0, st[8], sp = 0;
			st[sp++] = c;
			while(sp)
			{
				const int b = st[--sp];
				if(t.is_leaf(b)) { if(tri_at < ref_limit) { tri_indices[tri_at] = t.tri(b); placed(t, tri_at, b); } ++tri_at; ++cnt; }
				else if(sp <= 6) { st[sp++] = t.left(b); st[sp++] = t.right(b); }
			}
			meta[i] = (cnt == 1 ? 0x20u : cnt == 2 ? 0x60u : 0xe0u) | off;
		}
		else
		{
			const uint32_t widx = node_at - it.node_base;
			++node_at;
			widx_of[in_slot[i]] = (int)widx;
			meta[i] = (1u << 5) | (widx + 24u);
			imask |= 1u << widx;
		}
	}
	rec[kNodeExp / 4] = imask << 24;
	rec[kNodeChildBase / 4] = it.node_base;
	rec[kNodeTriBase / 4] = it.tri_base;
	rec[kNodeMeta / 4] = (meta[0] & 255u) | (meta[1] & 255u) << 8 | (meta[2] & 255u) << 16 | (meta[3] & 255u) << 24;
	rec[kNodeMeta / 4 + 1] = (meta[4] & 255u) | (meta[5] & 255u) << 8 | (meta[6] & 255u) << 16 | (meta[7] & 255u) << 24;
	// the runs of the inner children, in gather order, behind this node's own children and references
	int n_kids = 0;
	for(int i = 0; i < n_child; ++i)
	{
		if(t.row(child[i])[1].type != kInternal) continue;
		kids[n_kids++] = WideItem{(int32_t)(it.node_base + (uint32_t)widx_of[i]), child[i], node_at, tri_at};
		node_at += t.wide_below(child[i]) - 1u;
		tri_at += (uint32_t)t.tri_count(child[i]);
	}
	return n_kids;
}
template <class Tree> ADYPT_HOST_DEVICE int lbvh_emit_node(const Tree &t, const WideItem &it, uint32_t rec[20], int32_t *tri_indices, uint32_t ref_limit, WideItem kids[8])
{
	return lbvh_emit_node(t, it, rec, tri_indices, ref_limit, kids, LbvhNobody{});
}

}  // namespace adypt
