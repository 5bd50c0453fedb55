// The root card: node 0 of the CWBVH8 decoded ONCE per scene change into the form k_path's shading round wants (path.hpp), so that a new ray is
// tested against the root's eight boxes where all 64 lanes are busy — plain fused multiply-adds on scalar operands, no byte conversions, no per-ray
// decoding of the meta bytes — and starts its traversal past the root visit.  THE definition for host (adypt_decode_root_card, tests) and device
// (k_root_card, tracer.hip): no HIP needed (a host compiler may include it), integer work and exact byte -> binary32 conversions only.
//
// The node (80 bytes = 20 words, host/common.hpp NodeRec): w0..w2 the origin p, w3 = ex | ey << 8 | ez << 16 | imask << 24, w4 child_base, w5 tri_base,
// w6 w7 the meta bytes of slots 0..7, then per axis the quantised planes, 8 bytes each: w8 w9 qlo x, w10 w11 qlo y, w12 w13 qlo z, w14 w15 qhi x,
// w16 w17 qhi y, w18 w19 qhi z.  What section D of the trip (traverse_trip.inc) derives from them per visit is what the card holds.
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

enum { RC_LOX = 0, RC_HIX, RC_LOY, RC_HIY, RC_LOZ, RC_HIZ };

struct RootCard {
	float q[8][6];          // per child: float(q) of qlo x, qhi x, qlo y, qhi y, qlo z, qhi z — exactly the values v_cvt_f32_ubyteN yields
	float scale[3];         // exp_byte<0..2>(w3): the exponent bytes as binary32 exponent fields, 2^(e - 127)
	float origin[3];        // w0..w2
	uint32_t child_base;    // w4: what the visit leaves in ng_x
	uint32_t tri_base;      // w5: ... in tg_x
	uint32_t imask;         // w3 >> 24: the low byte of ng_y after the visit
	uint32_t inner_only;    // 1: every occupied slot of the root is an internal child with child bits 001 — the visit raises only bits 24..31 of the hit mask
	uint32_t enabled;       // inner_only and the feature is allowed (ADYPT_ROOT_CARD): k_path's rays start past the root
	uint32_t pad;
	// per child, one byte each, as section D derives them (byte j & 3 of word j >> 2: words, so that the device reads them with scalar loads)
	uint32_t is_inner4[2];   // 1: the slot is an internal child,
	uint32_t bit_index4[2];  // the shift count before the octant is applied (meta & 31: 24 + slot for an internal child),
	uint32_t child_bits4[2]; // and what is shifted ((meta >> 5) & 7; 0 = empty slot: nothing is raised)
};
static_assert(sizeof(RootCard) == 264, "RootCard: the layout k_path reads with scalar loads");

ADYPT_HOST_DEVICE void decode_root_card(const uint32_t node[20], bool allow, RootCard *c)
{
	bool inner_only = true;
	for(int w = 0; w < 2; ++w) c->is_inner4[w] = c->bit_index4[w] = c->child_bits4[w] = 0u;
	for(int j = 0; j < 8; ++j)
	{
		const int w = j >> 2, sh = 8 * (j & 3);
		for(int k = 0; k < 6; ++k)
		{
			// (k: lox hix loy hiy loz hiz -> plane 0 3 1 4 2 5 of the node)
			const int plane = (k >> 1) + 3 * (k & 1);
			c->q[j][k] = (float)((node[8 + 2 * plane + w] >> sh) & 0xffu);
		}
		const uint32_t m = (node[6 + w] >> sh) & 0xffu;
		const bool inner = ((m & (m << 1)) & 0x10u) != 0u;
		c->is_inner4[w] |= (inner ? 1u : 0u) << sh;
		c->bit_index4[w] |= (m & 31u) << sh;
		c->child_bits4[w] |= ((m >> 5) & 7u) << sh;
		if(m != 0u && !(inner && (m >> 5) == 1u)) inner_only = false;
	}
	for(int k = 0; k < 3; ++k)
	{
		const uint32_t bits = ((node[3] >> (8 * k)) & 0xffu) << 23;
		__builtin_memcpy(&c->scale[k], &bits, 4);
		__builtin_memcpy(&c->origin[k], &node[k], 4);
	}
	c->child_base = node[4];
	c->tri_base = node[5];
	c->imask = node[3] >> 24;
	c->inner_only = inner_only ? 1u : 0u;
	c->enabled = inner_only && allow ? 1u : 0u;
	c->pad = 0u;
}

}  // namespace adypt
