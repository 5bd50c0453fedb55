// adypt_bvh_refit (include/adypt_host.h): the boxes of a CWBVH8 recomputed for moved triangles, in place, on the host.  The rule is
// ../device/refit.hpp, the order ../device/refit_plan.hpp — the texts the device path (refit.hip) compiles too.
#include "builders.hpp"
#include "../device/refit_plan.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

using namespace adypt;

int adypt_bvh_refit(void *nodes, int64_t n_nodes, const int32_t *tri_indices, int64_t n_refs, const void *triangles, int64_t n_tris)
{
	return bvh_refit_boxes(nodes, n_nodes, tri_indices, n_refs, triangles, n_tris, nullptr);
}

int adypt::bvh_refit_boxes(void *nodes_, int64_t n_nodes, const int32_t *tri_indices, int64_t n_refs, const void *triangles, int64_t n_tris, const RefitBox *ref_boxes)
{
	if(!nodes_ || !triangles || n_nodes <= 0 || n_refs < 0 || n_tris <= 0 || (n_refs > 0 && !tri_indices)) { set_host_error("adypt_bvh_refit: null or empty argument"); return ADYPT_E_INVALID; }
	for(int64_t r = 0; r < n_refs; ++r)
		if(tri_indices[r] < 0 || tri_indices[r] >= n_tris) { set_host_error("adypt_bvh_refit: tri_indices[" + std::to_string(r) + "] out of range"); return ADYPT_E_INVALID; }
	RefitPlan plan;
	std::string why;
	if(!plan_refit(nodes_, n_nodes, n_refs, &plan, &why)) { set_host_error("adypt_bvh_refit: " + why); return ADYPT_E_INVALID; }
	uint8_t *nodes = (uint8_t *)nodes_;
	const TriRec *tris = (const TriRec *)triangles;
	std::vector<RefitBox> boxes((size_t)n_nodes);
	for(int l = plan.levels() - 1; l >= 0; --l)
		for(int64_t k = plan.level_begin[(size_t)l]; k < plan.level_begin[(size_t)l + 1]; ++k)
		{
			const int32_t i = plan.order[(size_t)k];
			uint8_t *n = nodes + (size_t)i * kNodeBytes;
			uint32_t child_base, tri_base, word3;
			memcpy(&child_base, n + kNodeChildBase, 4);
			memcpy(&tri_base, n + kNodeTriBase, 4);
			memcpy(&word3, n + kNodeExp, 4);
			RefitBox slot[8], box = refit_empty_box();
			bool any = false;
			for(int s = 0; s < 8; ++s)
			{
				const uint32_t meta = n[kNodeMeta + s];
				const int kind = refit_slot_kind(meta);
				slot[s] = refit_empty_box();
				if(kind == kSlotInternal) slot[s] = boxes[(size_t)child_base + refit_child_offset(meta)];
				else if(kind == kSlotLeaf)
					for(int r = 0; r < refit_leaf_count(meta); ++r)
					{
						const size_t at = (size_t)tri_base + refit_leaf_offset(meta) + (size_t)r;
						if(ref_boxes) { slot[s] = refit_union(slot[s], ref_boxes[at]); continue; }
						float p[9];
						memcpy(p, tris[tri_indices[at]].p, sizeof(p));
						slot[s] = refit_union(slot[s], refit_triangle_box(p));
					}
				if(kind != kSlotEmpty) { box = refit_union(box, slot[s]); any = true; }
			}
			boxes[(size_t)i] = box;
			if(!any) continue;
			float p[3];
			uint32_t e[3];
			refit_header(box, word3, p, &word3, e);
			memcpy(n, p, 12);
			memcpy(n + kNodeExp, &word3, 4);
			for(int s = 0; s < 8; ++s)
			{
				if(n[kNodeMeta + s] == 0) continue;
				uint8_t q[6];
				refit_slot_bytes(box, e, slot[s], q);
				for(int a = 0; a < 6; ++a) n[kNodeQuant + a * 8 + s] = q[a];
			}
		}
	return ADYPT_OK;
}
