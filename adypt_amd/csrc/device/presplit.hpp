// Splitting large triangles into several references before the PLOC build (Ernst and Greiner, "Early split clipping for bounding volume hierarchies",
// 2007; Karras and Aila, "Fast parallel construction of high-quality bounding volume hierarchies", 2013, section 4): THE definition for host
// (adypt_presplit_refs, adypt_bvh_build_ploc_split) and device (build.hip, adypt_rebuild_bvh_ploc_split).  No HIP needed (a host compiler may include
// it), binary32, the operations in the order written, no fma and no libm — tests/presplit_truth.py restates it in numpy float32.
//
// Thresholds.  S = cut_area of the union of every triangle's refit_triangle_box (order-free); A_l = S * 2^-l for l = 0 .. kSplitLevels - 1.
// Cells.  A triangle's root cell is its refit_triangle_box, at depth 0.  A cell is cut at mid = (lo + hi) * 0.5f of its longest axis (the first axis
// wins ties) into the low half [lo, mid] and the high half [mid, hi]; a half's box is presplit_clip(triangle, half): the triangle clipped against the
// half's six planes (Sutherland-Hodgman: x lo, x hi, y lo, y hi, z lo, z hi; a vertex on a plane is inside; an edge a -> b, in the polygon's order,
// that changes sides gives the point a + t * (b - a) with t = (plane - a_k) / (b_k - a_k), whose coordinate k is the plane itself; the polygon holds
// at most 9 vertices — a convex one never has more — and one beyond the ninth is dropped), the
// min / max of that polygon by refit_min / refit_max, widened per axis by pad_k = 2^-20 * max |v_k| over the triangle's three vertices, then clamped to
// the half and to the triangle's box.  The clip is empty when no vertex is left.  So a child's box lies inside its parent's, areas never grow on the
// way down (the binary32 operations of cut_area are monotone), and the union of the two children contains the part of the triangle inside the parent.
// The pad covers the rounding of the crossing points: t is within 3 half-ulps of the real quotient, b - a, the product and the sum are one rounding
// each of values of at most 2 max |v_k|, so a crossing point is within about 8 * 2^-24 * max |v_k| of the real one (a term-by-term bound); 2^-20 is
// twice that.  Measured (tests/test_presplit_definition.py test_containment: a binary64 clip of the same cells, 2 000 random triangles with coordinates
// up to 1e3, and the beams): the unpadded binary32 box is short by at most 4.44 * 2^-24 * max |v_k|, so the pad of 16 * 2^-24 has a margin of 3.6 and
// was not enlarged.
// A cell is splittable when its depth is below kSplitMaxDepth and neither half's clip is empty.
// Counts.  At level l a cell splits iff cut_area(cell) > A_l and it is splittable; a triangle's references are the leaves of that walk, depth first,
// low half first.  Because areas never grow, the cells that split at level l are those of the full walk (down to A_23) whose bin  b = the smallest l
// with area > A_l  is <= l: every splitting cell of the full walk adds 1 to hist[b], and extra(l) = hist[0] + .. + hist[l] references are added at
// level l — integer sums, whatever the order.  The chosen level is the largest l with extra(l) <= floor(split_budget * n) (the product in binary64);
// -1, and nothing is split, when there is none and when the budget is 0 (the stage is then not run at all).
// References.  Triangles in index order, a triangle's leaves in walk order: reference r = the exclusive scan of the per-triangle counts + the leaf's
// ordinal; ref_tri[r] is the triangle, ref_box[r] the leaf's box — the whole refit_triangle_box for a triangle with one reference.
// Keys.  A reference of an unsplit triangle has lbvh_centroid of the triangle, a split one (lo + hi) * 0.5f of its box; the centroid box is taken over
// the references; the key is code << 32 | r.  Where nothing is split (level -1, or extra(level) == 0) the keys, the sort and the whole tree are
// adypt_bvh_build_ploc's, and the tree carries no reference boxes.
// Downstream.  The binary tree's leaf boxes are ref_box; tri_indices gets ref_tri; the exact box of a leaf slot in the refit that ends the build is the
// union of its references' ref_box.  The cut, the layout and the quantisation are untouched.
#pragma once
#include "refit.hpp"
#include "wide_cut.hpp"

namespace adypt {

constexpr int kSplitLevels = 24, kSplitMaxDepth = 6;
constexpr int kSplitMaxRefs = 1 << kSplitMaxDepth; // of one triangle
constexpr int kSplitPolygon = 9;

ADYPT_HOST_DEVICE float presplit_threshold(float s, int level) { return s * refit_float((uint32_t)(127 - level) << 23); }
ADYPT_HOST_DEVICE float presplit_abs(float v) { return v < 0.0f ? -v : v; }
// v[k] by selects: an index known only at run time would put the array into scratch memory on the device
ADYPT_HOST_DEVICE float presplit_pick(const float v[3], int k) { return k == 0 ? v[0] : k == 1 ? v[1] : v[2]; }

// pad[k] = 2^-20 * max |v_k|
ADYPT_HOST_DEVICE void presplit_pad(const float *p, float pad[3])
{
	for(int k = 0; k < 3; ++k)
	{
		float m = presplit_abs(p[k]);
		const float b = presplit_abs(p[3 + k]), c = presplit_abs(p[6 + k]);
		m = m < b ? b : m;
		m = m < c ? c : m;
		pad[k] = m * refit_float((uint32_t)(127 - 20) << 23);
	}
}

// one plane of Sutherland-Hodgman: the n vertices of polygon `from` -> polygon `to`, the number of vertices left.  keep_above: inside is v_k >= plane,
// else v_k <= plane.  Work: see presplit_walk
template <class Work> ADYPT_HOST_DEVICE int presplit_clip_plane(Work &w, int from, int n, int k, float plane, bool keep_above, int to)
{
	int m = 0;
	for(int i = 0; i < n; ++i)
	{
		const int h = i == 0 ? n - 1 : i - 1;
		const float a[3] = {w.v(from, h, 0), w.v(from, h, 1), w.v(from, h, 2)}, b[3] = {w.v(from, i, 0), w.v(from, i, 1), w.v(from, i, 2)};
		const float ak = presplit_pick(a, k), bk = presplit_pick(b, k);
		const bool a_in = keep_above ? ak >= plane : ak <= plane, b_in = keep_above ? bk >= plane : bk <= plane;
		if(a_in != b_in)
		{
			const float t = (plane - ak) / (bk - ak);
			if(m < kSplitPolygon) { for(int c = 0; c < 3; ++c) w.v(to, m, c) = c == k ? plane : a[c] + t * (b[c] - a[c]); ++m; }
		}
		if(b_in && m < kSplitPolygon) { for(int c = 0; c < 3; ++c) w.v(to, m, c) = b[c]; ++m; }
	}
	return m;
}

// p: 9 floats; half: the box to clip against; whole: the triangle's box; pad: presplit_pad.  false: the clip is empty
template <class Work> ADYPT_HOST_DEVICE bool presplit_clip(Work &w, const float *p, const RefitBox &half, const RefitBox &whole, const float pad[3], RefitBox *out)
{
	int n = 3; // a plane adds at most one vertex: 3 + 6 = kSplitPolygon
	for(int i = 0; i < 3; ++i)
		for(int c = 0; c < 3; ++c) w.v(0, i, c) = p[i * 3 + c];
	for(int k = 0; k < 3; ++k)
	{
		n = presplit_clip_plane(w, 0, n, k, presplit_pick(half.lo, k), true, 1);
		n = presplit_clip_plane(w, 1, n, k, presplit_pick(half.hi, k), false, 0);
	}
	if(n == 0) return false;
	RefitBox r = refit_empty_box();
	for(int i = 0; i < n; ++i)
		for(int c = 0; c < 3; ++c) { const float v = w.v(0, i, c); r.lo[c] = refit_min(r.lo[c], v); r.hi[c] = refit_max(r.hi[c], v); }
	for(int c = 0; c < 3; ++c)
	{
		r.lo[c] = refit_max(refit_max(r.lo[c] - pad[c], half.lo[c]), whole.lo[c]);
		r.hi[c] = refit_min(refit_min(r.hi[c] + pad[c], half.hi[c]), whole.hi[c]);
	}
	*out = r;
	return true;
}

// the two children of a cell, or false where it is not splittable (the depth is the caller's to check)
template <class Work> ADYPT_HOST_DEVICE bool presplit_children(Work &w, const float *p, const RefitBox &cell, const RefitBox &whole, const float pad[3], RefitBox *low, RefitBox *high)
{
	const float e[3] = {cell.hi[0] - cell.lo[0], cell.hi[1] - cell.lo[1], cell.hi[2] - cell.lo[2]};
	int k = 0;
	if(e[1] > e[0]) k = 1;
	if(e[2] > presplit_pick(e, k)) k = 2;
	const float mid = (presplit_pick(cell.lo, k) + presplit_pick(cell.hi, k)) * 0.5f;
	RefitBox h = cell;
	for(int c = 0; c < 3; ++c) h.hi[c] = c == k ? mid : cell.hi[c];
	if(!presplit_clip(w, p, h, whole, pad, low)) return false;
	h = cell;
	for(int c = 0; c < 3; ++c) h.lo[c] = c == k ? mid : cell.lo[c];
	return presplit_clip(w, p, h, whole, pad, high);
}

// the bin of a cell that splits in the full walk: the smallest l with area > A_l (the caller knows area > A_(kSplitLevels - 1))
ADYPT_HOST_DEVICE int presplit_bin(float area, float s)
{
	int l = 0;
	while(l < kSplitLevels - 1 && !(area > presplit_threshold(s, l))) ++l;
	return l;
}

// The walk of one triangle at `threshold`.  Work: the memory of the walk, indexed at run time (plain arrays on the host, LDS on the device, where such
// arrays in registers would go to scratch) —
//     void put(int depth, const RefitBox &), RefitBox get(int depth)     the high halves that wait for their turn, one per depth 1 .. kSplitMaxDepth
//     float &v(int polygon, int vertex, int axis)                         two polygons of kSplitPolygon vertices for the clip
// Visit:  void split(float area)  for every cell that splits,  void leaf(const RefitBox &, int ordinal).  Returns the number of leaves.
template <class Work, class Visit> ADYPT_HOST_DEVICE int presplit_walk(const float *p, float threshold, Work &work, Visit &visit)
{
	const RefitBox whole = refit_triangle_box(p);
	float pad[3];
	presplit_pad(p, pad);
	RefitBox cell = whole;
	int depth = 0, leaves = 0;
	uint32_t waiting = 0; // bit d: a high half waits at depth d
	for(;;)
	{
		if(depth < kSplitMaxDepth)
		{
			const float area = cut_area(cell.lo, cell.hi);
			RefitBox low, high;
			if(area > threshold && presplit_children(work, p, cell, whole, pad, &low, &high))
			{
				visit.split(area);
				++depth;
				work.put(depth, high);
				waiting |= 1u << depth;
				cell = low;
				continue;
			}
		}
		visit.leaf(cell, leaves);
		++leaves;
		if(!waiting) return leaves;
		depth = 31 - __builtin_clz(waiting); // the deepest one is the one put last
		waiting &= ~(1u << depth);
		cell = work.get(depth);
	}
}

// The bin of a triangle's root cell if it splits in the full walk, else -1.  Every split of a level is counted in extra(l), the root cells' among them,
// so the level chosen is at most the largest l at which the root cells alone stay inside the budget: the builders count the root cells first (two
// clips per triangle) and walk only down to that level for the histogram — the bins up to it are exact, the ones below it are never looked at.
template <class Work> ADYPT_HOST_DEVICE int presplit_root_bin(const float *p, float s, Work &work)
{
	const RefitBox whole = refit_triangle_box(p);
	const float area = cut_area(whole.lo, whole.hi);
	if(!(area > presplit_threshold(s, kSplitLevels - 1))) return -1;
	float pad[3];
	presplit_pad(p, pad);
	RefitBox low, high;
	return presplit_children(work, p, whole, whole, pad, &low, &high) ? presplit_bin(area, s) : -1;
}

// the chosen level from the histogram: the largest l <= top with hist[0] + .. + hist[l] <= allowed, or -1; *extra: the references it adds
inline int presplit_level(const uint64_t hist[kSplitLevels], int64_t allowed, int64_t *extra, int top = kSplitLevels - 1)
{
	int level = -1;
	int64_t sum = 0;
	*extra = 0;
	for(int l = 0; l <= top; ++l)
	{
		sum += (int64_t)hist[l];
		if(sum > allowed) break;
		level = l;
		*extra = sum;
	}
	return level;
}
// floor(budget * n), the product in binary64
inline int64_t presplit_allowed(double budget, int64_t n) { return (int64_t)(budget * (double)n); }

// the centroid of a reference for its key
ADYPT_HOST_DEVICE float presplit_centroid(const RefitBox &box, int k) { return (box.lo[k] + box.hi[k]) * 0.5f; }

}  // namespace adypt
