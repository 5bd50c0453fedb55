// Refitting a CWBVH8 to moved triangles: the topology (meta, imask, child_base, tri_base, the reference order) stays, the boxes are recomputed bottom
// up.  THE definition for host (adypt_bvh_refit) and device (k_refit_nodes): no HIP needed (a host compiler may include it), binary32, the operations
// in the order written, no fma and no libm — tests/refit_truth.py restates these lines in numpy float32 and is bit-exact.
//
// Slots (as the builder writes them, host/wide_builder.cpp emit()): meta == 0 empty; (meta >> 5) == 1 and (meta & 31) >= 24 an internal child at node
// child_base + (meta & 31) - 24; otherwise a leaf whose top bits 001 / 011 / 111 mean 1 / 2 / 3 references from tri_base + (meta & 31).
//
// Exact boxes (a side array, not part of the node): a leaf slot's box bounds the WHOLE triangle of each of its references (also where the builder had
// clipped a spatially split one), an internal slot's box is the child node's exact box — never the dequantised one, so nothing widens level by level —
// and a node's box is the union of its occupied slots.  min and max order -0 below +0, so a union does not depend on the order it is taken in (the
// device takes it across lanes) and is exact to the bit.
//
// The node record: p = box.lo; per axis cell = (hi - lo) * float(1 / 255) and the exponent byte = 0 for cell == 0, else the biased exponent of the
// smallest power of two >= cell, read from the bits (exponent field + 1 if the mantissa is not zero, kept in [1, 254]); per occupied slot and axis
// qlo = min(floor((c.lo - lo) / 2^e), 255), qhi = min(ceil((c.hi - lo) / 2^e), 255), both 0 where the byte is 0.  The bytes of empty slots and every other
// field stay.  A node without an occupied slot (the builder emits none) stays as it is and its exact box is empty (+inf, -inf).
// With unmoved triangles and no spatial splits this is the builder's record; the builder's ceil(log2f(cell)) differs only where libm rounds a value just
// above a power of two down, and there this rule is the conservative one.
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

constexpr int kNodeBytes = 80;
// byte offsets in the 80-byte node (host/common.hpp NodeRec)
constexpr int kNodeExp = 12, kNodeChildBase = 16, kNodeTriBase = 20, kNodeMeta = 24, kNodeQuant = 32; // quantised bytes: [qlo x y z, qhi x y z][slot]

struct RefitBox { float lo[3], hi[3]; };

ADYPT_HOST_DEVICE uint32_t refit_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
ADYPT_HOST_DEVICE float refit_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
ADYPT_HOST_DEVICE float refit_inf() { return refit_float(0x7f800000u); }

// -0 < +0: the result of a chain of these does not depend on its order
ADYPT_HOST_DEVICE float refit_min(float a, float b) { return (b < a || (b == a && (refit_bits(b) >> 31))) ? b : a; }
ADYPT_HOST_DEVICE float refit_max(float a, float b) { return (a < b || (a == b && !(refit_bits(b) >> 31))) ? b : a; }

ADYPT_HOST_DEVICE RefitBox refit_empty_box()
{
	const float inf = refit_inf();
	return RefitBox{{inf, inf, inf}, {-inf, -inf, -inf}};
}
ADYPT_HOST_DEVICE RefitBox refit_union(const RefitBox &a, const RefitBox &b)
{
	RefitBox r;
	for(int k = 0; k < 3; ++k) { r.lo[k] = refit_min(a.lo[k], b.lo[k]); r.hi[k] = refit_max(a.hi[k], b.hi[k]); }
	return r;
}
// p: 9 floats, the three vertices
ADYPT_HOST_DEVICE RefitBox refit_triangle_box(const float *p)
{
	RefitBox r;
	for(int k = 0; k < 3; ++k)
	{
		r.lo[k] = refit_min(p[k], refit_min(p[3 + k], p[6 + k]));
		r.hi[k] = refit_max(p[k], refit_max(p[3 + k], p[6 + k]));
	}
	return r;
}

enum RefitSlot { kSlotEmpty = 0, kSlotInternal = 1, kSlotLeaf = 2 };
ADYPT_HOST_DEVICE int refit_slot_kind(uint32_t meta) { return meta == 0 ? kSlotEmpty : ((meta >> 5) == 1u && (meta & 31u) >= 24u) ? kSlotInternal : kSlotLeaf; }
ADYPT_HOST_DEVICE uint32_t refit_child_offset(uint32_t meta) { return (meta & 31u) - 24u; }   // internal: the child is node child_base + this
ADYPT_HOST_DEVICE uint32_t refit_leaf_offset(uint32_t meta) { return meta & 31u; }            // leaf: its references start at tri_base + this
// leaf: 1 / 2 / 3 for the top bits 001 / 011 / 111; 0 for anything else (no builder writes it: refit_plan.hpp refuses such a node)
ADYPT_HOST_DEVICE int refit_leaf_count(uint32_t meta) { const uint32_t b = meta >> 5; return b == 1u ? 1 : b == 3u ? 2 : b == 7u ? 3 : 0; }

ADYPT_HOST_DEVICE float refit_cell(float lo, float hi) { return (hi - lo) * float(1.0 / 255); }
ADYPT_HOST_DEVICE uint32_t refit_exponent(float cell)
{
	if(cell == 0.0f) return 0u;
	const uint32_t u = refit_bits(cell);
	uint32_t e = ((u >> 23) & 255u) + ((u & 0x7fffffu) ? 1u : 0u);
	e = e < 1u ? 1u : e;
	return e > 254u ? 254u : e;
}
// floor (up == false) or ceil (up == true) of x / 2^(e - 127), at most 255; 0 where the exponent byte is 0.  x >= 0: a slot's box lies in its node's.
ADYPT_HOST_DEVICE uint32_t refit_quantise(float x, uint32_t e, bool up)
{
	if(e == 0u) return 0u;
	const float q = x / refit_float(e << 23);
	if(!(q < 255.0f)) return 255u;
	const float f = (float)(int)q;
	return (uint32_t)(int)f + ((up && f < q) ? 1u : 0u);
}

// The new bytes of a node whose exact box is `box`: the header's 16 bytes (p and the three exponent bytes; imask is kept) ...
ADYPT_HOST_DEVICE void refit_header(const RefitBox &box, uint32_t old_word3, float p[3], uint32_t *word3, uint32_t e[3])
{
	for(int k = 0; k < 3; ++k) { p[k] = box.lo[k]; e[k] = refit_exponent(refit_cell(box.lo[k], box.hi[k])); }
	*word3 = e[0] | e[1] << 8 | e[2] << 16 | (old_word3 & 0xff000000u);
}
// ... and the six quantised bytes of one occupied slot whose exact box is `c`: q[0..2] = qlo x y z, q[3..5] = qhi x y z
ADYPT_HOST_DEVICE void refit_slot_bytes(const RefitBox &box, const uint32_t e[3], const RefitBox &c, uint8_t q[6])
{
	for(int k = 0; k < 3; ++k)
	{
		q[k] = (uint8_t)refit_quantise(c.lo[k] - box.lo[k], e[k], false);
		q[3 + k] = (uint8_t)refit_quantise(c.hi[k] - box.lo[k], e[k], true);
	}
}

}  // namespace adypt
