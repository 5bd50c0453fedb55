// The SAH cost of a CWBVH8 as the traversal sees it, from the quantised child boxes of the 80-byte nodes alone: THE definition for host (adypt_bvh_cost)
// and device (k_tree_cost, adypt_get_tree_cost).  No HIP needed (a host compiler may include it), binary32, the operations in the order written, no
// fma and no libm — tests/tree_cost_truth.py restates these lines in numpy float32 / uint64 and is bit-exact.
//
// Slot extents.  For every occupied slot (meta != 0; the slots are decoded as refit.hpp says) of every node the extent per axis is
// float(max(qhi - qlo, 0)) * 2^(e - 127), e the node's exponent byte of that axis (0 where the byte is 0): an integer below 256 times a power of two,
// which is exact.  The slot's area is cut_area's expression (wide_cut.hpp): (ex * (ey + ez) + ey * ez) * 2.
// Root area A.  The same expression on the union of node 0's occupied slots: per axis min of qlo and max of qhi (integers, whatever the order) times
// node 0's scale.
// Per slot.  r = area / A, one binary32 division; q = (uint64)(r * 2^30), cut off (the product is exact: a power of two).
// Two integer sums over all slots of all nodes: inner_q = the sum of q over the slots that hold a child node, leaf_q = the sum of q * (references in
// the slot: 1, 2 or 3) over the leaf slots.  Integer sums do not depend on their order: the device adds with atomics and gets the host's bits.
// Cost, in binary64, from the two integers, on both sides: node_sah * (1 + inner_q / 2^30) + triangle_sah * leaf_q / 2^30 — the expected number of
// node visits of a random ray that hits the root, times node_sah (the 1 is the root's own visit), plus its expected triangle tests times triangle_sah.
// Invalid trees: A that is not a positive finite number (a root without area: every triangle at one point), an r that is NaN or >= 4 (no builder and
// no refit here makes a child four times the root), more than 2^26 nodes.
// Bounds.  q < 2^32 because r < 4; with at most 3 references per slot and at most 2^26 * 8 = 2^29 slots each sum stays below 3 * 2^32 * 2^29 < 2^63.
// Cutting q off loses less than 2^-30 per slot: inner_q / 2^30 and leaf_q / 2^30 are short of the sums of the exact r by at most slots * 2^-30 and
// 3 * slots * 2^-30, so the cost is low by at most (node_sah + 3 triangle_sah) * slots * 2^-30 — 5e-4 for a million nodes at the default costs.
#pragma once
#include "refit.hpp"

namespace adypt {

constexpr int64_t kCostMaxNodes = (int64_t)1 << 26;
constexpr float kCostUnit = 1073741824.0f; // 2^30
constexpr float kCostMaxRatio = 4.0f;

// 2^(e - 127) of an exponent byte; 0 for the byte 0
ADYPT_HOST_DEVICE float cost_scale(uint32_t e) { return refit_float(e << 23); }
// the area of a quantised box: q[0..2] = qlo x y z, q[3..5] = qhi x y z, e the three exponent bytes
ADYPT_HOST_DEVICE float cost_area(const uint32_t q[6], const uint32_t e[3])
{
	float ext[3];
	for(int k = 0; k < 3; ++k)
	{
		const int d = (int)q[3 + k] - (int)q[k];
		ext[k] = (float)(d > 0 ? d : 0) * cost_scale(e[k]);
	}
	return (ext[0] * (ext[1] + ext[2]) + ext[1] * ext[2]) * 2.0f;
}
// the six quantised bytes of slot s and the three exponent bytes of the 80-byte node at `node`
ADYPT_HOST_DEVICE void cost_slot_bytes(const uint8_t *node, int s, uint32_t q[6], uint32_t e[3])
{
	for(int a = 0; a < 6; ++a) q[a] = node[kNodeQuant + a * 8 + s];
	for(int k = 0; k < 3; ++k) e[k] = node[kNodeExp + k];
}
// byte b of a node given as its 20 little-endian words (the device holds node 0 in registers)
ADYPT_HOST_DEVICE uint32_t cost_byte(const uint32_t *w, int b) { return (w[b >> 2] >> ((b & 3) * 8)) & 255u; }
// A: the area of the union of the occupied slots of the node given as its 20 words (node 0)
ADYPT_HOST_DEVICE float cost_root_area(const uint32_t *w)
{
	uint32_t u[6] = {255u, 255u, 255u, 0u, 0u, 0u}, e[3];
	for(int s = 0; s < 8; ++s)
	{
		if(cost_byte(w, kNodeMeta + s) == 0) continue;
		for(int k = 0; k < 3; ++k)
		{
			const uint32_t lo = cost_byte(w, kNodeQuant + k * 8 + s), hi = cost_byte(w, kNodeQuant + (3 + k) * 8 + s);
			u[k] = lo < u[k] ? lo : u[k];
			u[3 + k] = hi > u[3 + k] ? hi : u[3 + k];
		}
	}
	for(int k = 0; k < 3; ++k) e[k] = cost_byte(w, kNodeExp + k);
	return cost_area(u, e);
}
ADYPT_HOST_DEVICE bool cost_root_valid(float A) { return A > 0.0f && A < refit_inf(); }
// One occupied slot's share of the two sums; ok == false, and no share, for an r that is NaN or >= 4
struct CostShare { uint64_t inner_q, leaf_q; bool ok; };
ADYPT_HOST_DEVICE CostShare cost_slot(uint32_t meta, float area, float A)
{
	const float r = area / A;
	if(!(r < kCostMaxRatio)) return CostShare{0, 0, false};
	const uint64_t q = (uint64_t)(uint32_t)(r * kCostUnit); // (r < 4: below 2^32)
	const bool inner = refit_slot_kind(meta) == kSlotInternal;
	return CostShare{inner ? q : 0, inner ? 0 : q * (uint64_t)refit_leaf_count(meta), true};
}
// the cost from the two sums, in binary64
inline double cost_value(double node_sah, double triangle_sah, uint64_t inner_q, uint64_t leaf_q)
{
	const double unit = 1073741824.0;
	return node_sah * (1.0 + (double)inner_q / unit) + triangle_sah * ((double)leaf_q / unit);
}

}  // namespace adypt
