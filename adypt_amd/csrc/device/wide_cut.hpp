// Where a binary BVH is cut into 8-wide nodes: the SAH dynamic program of the collapse ("i in 1..7 roots of a forest cut from this subtree"), the
// children it gives a wide node and their assignment to the eight slots.  THE arithmetic for the host's collapse (host/wide_builder.cpp) and for the
// device's (build.hip): no HIP needed, binary32, the operations in the order written, no fma and no libm.  What the decisions restate is told in
// host/wide_builder.cpp; the golden .bvh files pin them.
//
// A tree is anything with   int left(int n), int right(int n), const CutRow &row(int n), uint32_t wide_below(int n)   — the host's is laid out in
// pre-order (right child = n + 1), the device's is Karras's radix tree (lbvh.hpp).  The walks below keep a stack of their own: a forest of i <= 8 roots
// is cut by at most 7 distributions, so 8 entries hold it.  Rows that are not the DP's (shares outside 1..7, more roots than 8) end a walk instead of
// leaving its arrays: the result is then wrong, never a stray access.
#pragma once
#include <cstdint>

#ifndef ADYPT_HOST_DEVICE
#ifdef __HIPCC__
#define ADYPT_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define ADYPT_HOST_DEVICE inline
#endif
#endif

namespace adypt {

enum CutType : uint8_t { kInternal = 0, kLeaf = 1, kDistribute = 2 };
struct Cut { float sah; uint8_t type; uint8_t split[2]; uint8_t pad; }; // 8 B: 56 B of DP state per binary node
struct CutRow {
	Cut c[7];
	ADYPT_HOST_DEVICE Cut &operator[](int i) { return c[i - 1]; }
	ADYPT_HOST_DEVICE const Cut &operator[](int i) const { return c[i - 1]; }
};

constexpr float kCutMax = 3.402823466e+38f; // FLT_MAX

// Box::area (host/common.hpp)
ADYPT_HOST_DEVICE float cut_area(const float lo[3], const float hi[3])
{
	const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
	return (ex * (ey + ez) + ey * ez) * 2.0f;
}

// the row of a binary leaf (one reference)
ADYPT_HOST_DEVICE void cut_leaf_row(float area, float triangle_sah, CutRow &dp)
{
	for(int i = 1; i <= 7; ++i) { dp[i].sah = (triangle_sah * 1) * area; dp[i].type = kLeaf; dp[i].split[0] = dp[i].split[1] = 0; dp[i].pad = 0; }
}

// the row of an inner binary node with `tc` references below it from its children's rows; strict '<' everywhere (the first minimum wins).
// false: no split of the eight slots costs less than FLT_MAX (costs that overflow, or are NaN); the row then names the split 4 + 4, so that a walk over
// it stays inside the rows, and the caller refuses the tree (the device builder and the host's collapse both do)
ADYPT_HOST_DEVICE bool cut_inner_row(float area, int tc, float triangle_sah, float node_sah_, const CutRow &L, const CutRow &R, CutRow &dp)
{
	{
		float c_leaf = tc <= 3 ? area * (triangle_sah * tc) : kCutMax;
		float c_int = kCutMax;
		float node_sah = area * (node_sah_ * 8);
		dp[1].split[0] = dp[1].split[1] = 0;
		dp[1].pad = 0;
		for(int k = 1; k < 8; ++k)
		{
			float v = node_sah + L[k].sah + R[8 - k].sah;
			if(v < c_int) { c_int = v; dp[1].split[0] = (uint8_t)k; dp[1].split[1] = (uint8_t)(8 - k); }
		}
		if(c_leaf < c_int) { dp[1].sah = c_leaf; dp[1].type = kLeaf; }
		else { dp[1].sah = c_int; dp[1].type = kInternal; }
	}
	const bool ok = dp[1].split[0] != 0;
	if(!ok) dp[1].split[0] = dp[1].split[1] = 4;
	for(int i = 2; i <= 7; ++i)
	{
		float c_dist = kCutMax;
		dp[i].split[0] = dp[i].split[1] = 0;
		dp[i].pad = 0;
		for(int k = 1; k < i; ++k)
		{
			float v = L[k].sah + R[i - k].sah;
			if(v < c_dist) { c_dist = v; dp[i].split[0] = (uint8_t)k; dp[i].split[1] = (uint8_t)(i - k); }
		}
		if(c_dist < dp[i - 1].sah) { dp[i].sah = c_dist; dp[i].type = kDistribute; }
		else dp[i] = dp[i - 1];
	}
	return ok;
}

// wide nodes emitted for the forest the DP cuts out of binary node n with a budget of i roots
template <class Tree> ADYPT_HOST_DEVICE uint32_t cut_forest_wide(const Tree &t, int n, int i)
{
	int node[8], share[8], sp = 0;
	uint32_t sum = 0;
	node[sp] = n; share[sp++] = i;
	while(sp)
	{
		--sp;
		const int m = node[sp], b = share[sp];
		if(b < 1 || b > 7) break;
		const Cut &c = t.row(m)[b];
		if(c.type != kDistribute) { sum += t.wide_below(m); continue; }
		if(sp > 6) break;
		node[sp] = t.right(m); share[sp++] = c.split[1];
		node[sp] = t.left(m); share[sp++] = c.split[0];
	}
	return sum;
}

// wide nodes emitted for binary node n as a direct child: itself + everything below (0 for a leaf cut); its row and its children's counts are known
template <class Tree> ADYPT_HOST_DEVICE uint32_t cut_wide_below(const Tree &t, int n)
{
	const Cut &c = t.row(n)[1];
	return c.type == kInternal ? 1u + cut_forest_wide(t, t.left(n), c.split[0]) + cut_forest_wide(t, t.right(n), c.split[1]) : 0u;
}

// the binary nodes that become the children of a wide node rooted at (n, i): the left child's share first, depth first
template <class Tree> ADYPT_HOST_DEVICE void cut_gather_children(const Tree &t, int n, int i, int *count, int out[8])
{
	int node[8], share[8], sp = 0;
	if(i < 1 || i > 7) return;
	{
		const Cut &c = t.row(n)[i];
		node[sp] = t.right(n); share[sp++] = c.split[1];
		node[sp] = t.left(n); share[sp++] = c.split[0];
	}
	while(sp)
	{
		--sp;
		const int m = node[sp], b = share[sp];
		if(b < 1 || b > 7 || *count > 7) break;
		const Cut &c = t.row(m)[b];
		if(c.type != kDistribute) { out[(*count)++] = m; continue; }
		if(sp > 6) break;
		node[sp] = t.right(m); share[sp++] = c.split[1];
		node[sp] = t.left(m); share[sp++] = c.split[0];
	}
}

// min-cost assignment of `n` rows (children) to 8 columns (slots), potentials method; slot_of[row] = column.  Costs that are NaN or reach 1e12 leave
// the search without a column to go on with (the host's collapse used to spin there): the children then take the slots in their order.
ADYPT_HOST_DEVICE void cut_assign_slots(const float cost[8][8], int n, int slot_of[8])
{
	const float INF = 1e12f;
	int match[9], way[9];     // match[col] = row matched to col (1-based, 0 = none)
	float u[9], v[9], minv[9];
	bool used[9];
	for(int j = 0; j < 9; ++j) { u[j] = 0.0f; v[j] = 0.0f; way[j] = 0; match[j] = 0; }
	for(int row = 1; row <= n; ++row)
	{
		match[0] = row;
		int j0 = 0;
		for(int j = 0; j < 9; ++j) { minv[j] = INF; used[j] = false; }
		do
		{
			used[j0] = true;
			int i0 = match[j0], j1 = 0;
			float delta = INF;
			for(int j = 1; j <= 8; ++j)
				if(!used[j])
				{
					float cur = cost[i0 - 1][j - 1] - u[i0] - v[j];
					if(cur < minv[j]) { minv[j] = cur; way[j] = j0; }
					if(minv[j] < delta) { delta = minv[j]; j1 = j; }
				}
			if(j1 == 0)
			{
				for(int r = 0; r < n; ++r) slot_of[r] = r;
				return;
			}
			for(int j = 0; j <= 8; ++j)
				if(used[j]) { u[match[j]] += delta; v[j] -= delta; }
				else minv[j] -= delta;
			j0 = j1;
		} while(match[j0] != 0);
		do
		{
			int j1 = way[j0];
			match[j0] = match[j1];
			j0 = j1;
		} while(j0);
	}
	for(int j = 1; j <= 8; ++j)
		if(match[j] != 0) slot_of[match[j] - 1] = j - 1;
}

// the cost of child box c (centre) in slot j of a node whose centre is pc: the signed offsets, x then y then z
ADYPT_HOST_DEVICE float cut_slot_cost(const float d[3], int j) { return ((j & 1) ? -d[0] : d[0]) + ((j & 2) ? -d[1] : d[1]) + ((j & 4) ? -d[2] : d[2]); }

}  // namespace adypt
