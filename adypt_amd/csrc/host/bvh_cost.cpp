// adypt_bvh_cost (include/adypt_host.h): the SAH cost of a CWBVH8 from its quantised child boxes, on the host.  The rule is ../device/tree_cost.hpp —
// the text the device path (refit.hip, k_tree_cost) compiles too.
#include "builders.hpp"
#include "../device/build_request.hpp"
#include "../device/tree_cost.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

using namespace adypt;

int adypt_bvh_cost(const void *nodes_, int64_t n_nodes, const adypt_bvh_params *params, adypt_tree_cost *out)
{
	if(!nodes_ || !out || n_nodes <= 0) { set_host_error("adypt_bvh_cost: null or empty argument"); return ADYPT_E_INVALID; }
	const adypt_bvh_params cfg = build_cfg(params);
	if(const char *why = sah_refused(cfg, refit_inf())) { set_host_error(std::string("adypt_bvh_cost: ") + why); return ADYPT_E_INVALID; }
	if(n_nodes > kCostMaxNodes) { set_host_error("adypt_bvh_cost: more than 2^26 nodes"); return ADYPT_E_INVALID; }
	const uint8_t *nodes = (const uint8_t *)nodes_;
	uint32_t root[kNodeBytes / 4];
	memcpy(root, nodes, kNodeBytes);
	const float A = cost_root_area(root);
	if(!cost_root_valid(A)) { set_host_error("adypt_bvh_cost: the root's box has no positive finite area"); return ADYPT_E_INVALID; }
	uint64_t inner_q = 0, leaf_q = 0;
	for(int64_t i = 0; i < n_nodes; ++i)
	{
		const uint8_t *n = nodes + (size_t)i * kNodeBytes;
		for(int s = 0; s < 8; ++s)
		{
			const uint32_t meta = n[kNodeMeta + s];
			if(meta == 0) continue;
			uint32_t q[6], e[3];
			cost_slot_bytes(n, s, q, e);
			const CostShare share = cost_slot(meta, cost_area(q, e), A);
			inner_q += share.inner_q;
			leaf_q += share.leaf_q;
			if(!share.ok)
			{
				set_host_error("adypt_bvh_cost: slot " + std::to_string(s) + " of node " + std::to_string(i) + " is not below four times the root's area");
				return ADYPT_E_INVALID;
			}
		}
	}
	out->cost = cost_value((double)cfg.node_sah, (double)cfg.triangle_sah, inner_q, leaf_q);
	out->inner_q = inner_q;
	out->leaf_q = leaf_q;
	out->n_nodes = n_nodes;
	return ADYPT_OK;
}
