// adypt_pose_triangles, adypt_pose_triangles_morph, adypt_morph_diff (include/adypt_host.h): triangles posed by morph weights and part or joint
// matrices, on the host.  The rule is ../device/pose.hpp — the text the device path (pose.hip, k_pose) compiles too.
#include "common.hpp"
#include "../device/pose.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

using namespace adypt;

namespace {

// a checked morph layer in the order the morph stage takes it
struct Morph {
	const float *deltas = nullptr, *weights = nullptr;
	const int32_t *targets = nullptr;
	std::vector<int32_t> order, offsets;
};

// what both entry points refuse of the matrix stage: the reason, or empty
std::string matrix_stage_refused(const void *triangles_in, int64_t n_tris, const int32_t *parts, const uint16_t *joints, const float *weights, const float *matrices,
                                 int32_t n_matrices, const void *triangles_out)
{
	const bool by_parts = parts != nullptr;
	if(n_tris < 0) return "n_tris is negative";
	if(!triangles_in || !triangles_out || !matrices) return "null argument";
	if(by_parts ? (joints || weights) : (!joints || !weights)) return "give either parts, or joints and weights";
	const char *why = pose_refuse_count(n_matrices);
	if(!why) why = by_parts ? pose_refuse_parts(parts, n_tris, n_matrices) : pose_refuse_skin(joints, weights, n_tris, n_matrices);
	if(!why) why = pose_refuse_matrices(matrices, n_matrices);
	return why ? why : "";
}

// everything has been checked; morph may be null
void pose_all(const void *triangles_in, int64_t n_tris, const int32_t *parts, const uint16_t *joints, const float *weights, const float *matrices, const Morph *morph,
              void *triangles_out)
{
	const bool by_parts = parts != nullptr;
	const uint8_t *in = (const uint8_t *)triangles_in;
	uint8_t *out = (uint8_t *)triangles_out;
	for(int64_t i = 0; i < n_tris; ++i)
	{
		TriRec t;
		memcpy(&t, in + i * sizeof(TriRec), sizeof(TriRec));
		TriRec posed = t; // (texture coordinates and material id stay)
		float acc[kMorphWords];
		memcpy(acc, &t, sizeof(acc)); // p0 p1 p2 n0 n1 n2
		if(morph)
			for(int32_t k = morph->offsets[(size_t)i]; k < morph->offsets[(size_t)i + 1]; ++k)
			{
				const int32_t e = morph->order[(size_t)k];
				const float w = morph->weights[morph->targets[e]];
				if(w == 0.0f) continue; // (the entry's deltas are never read)
				pose_morph(acc, w, morph->deltas + (size_t)e * kMorphWords);
			}
		for(int v = 0; v < 3; ++v)
		{
			float M[kPoseMatrixFloats] = {0};
			if(by_parts) memcpy(M, matrices + (size_t)parts[i] * kPoseMatrixFloats, sizeof(M));
			else
			{
				bool first = true;
				for(int k = 0; k < kPoseSlots; ++k)
				{
					const size_t slot = (size_t)i * kPoseTriSlots + v * kPoseSlots + k;
					if(weights[slot] == 0.0f) continue;
					pose_weigh(M, first, weights[slot], matrices + (size_t)joints[slot] * kPoseMatrixFloats);
					first = false;
				}
			}
			float p_out[3], n_out[3];
			pose_vertex(M, acc + 3 * v, acc + 9 + 3 * v, p_out, n_out);
			posed.p[v] = Vec3{p_out[0], p_out[1], p_out[2]};
			posed.n[v] = Vec3{n_out[0], n_out[1], n_out[2]};
		}
		memcpy(out + i * sizeof(TriRec), &posed, sizeof(TriRec));
	}
}

}  // namespace

int adypt_pose_triangles(const void *triangles_in, int64_t n_tris, const int32_t *parts, const uint16_t *joints, const float *weights, const float *matrices, int32_t n_matrices,
                         void *triangles_out)
{
	const std::string why = matrix_stage_refused(triangles_in, n_tris, parts, joints, weights, matrices, n_matrices, triangles_out);
	if(!why.empty()) { set_host_error("adypt_pose_triangles: " + why); return ADYPT_E_INVALID; }
	pose_all(triangles_in, n_tris, parts, joints, weights, matrices, nullptr, triangles_out);
	return ADYPT_OK;
}

int adypt_pose_triangles_morph(const void *triangles_in, int64_t n_tris, const int32_t *parts, const uint16_t *joints, const float *weights, const float *matrices, int32_t n_matrices,
                               const int32_t *triangle_of_entry, const int32_t *target_of_entry, const float *deltas, int64_t n_entries, const float *morph_weights,
                               int32_t n_targets, void *triangles_out)
{
	const std::string who = "adypt_pose_triangles_morph: ";
	std::string why = matrix_stage_refused(triangles_in, n_tris, parts, joints, weights, matrices, n_matrices, triangles_out);
	if(!why.empty()) { set_host_error(who + why); return ADYPT_E_INVALID; }
	if(!triangle_of_entry || !target_of_entry || !deltas || !morph_weights) { set_host_error(who + "null argument"); return ADYPT_E_INVALID; }
	Morph morph;
	const char *r = pose_refuse_morph_counts(n_entries, n_targets);
	if(!r) r = pose_refuse_morph_entries(triangle_of_entry, target_of_entry, deltas, n_entries, n_tris, n_targets);
	if(!r) r = pose_refuse_morph_weights(morph_weights, n_targets, n_targets);
	if(!r) r = pose_morph_order(triangle_of_entry, target_of_entry, n_entries, n_tris, morph.order, morph.offsets);
	if(r) { set_host_error(who + r); return ADYPT_E_INVALID; }
	morph.deltas = deltas; morph.weights = morph_weights; morph.targets = target_of_entry;
	pose_all(triangles_in, n_tris, parts, joints, weights, matrices, &morph, triangles_out);
	return ADYPT_OK;
}

int64_t adypt_morph_diff(const void *rest, const void *target, int64_t n_tris, int32_t *triangle_out, float *deltas_out)
{
	if(!rest || !target || n_tris < 0 || n_tris > kMorphMaxEntries) { set_host_error("adypt_morph_diff: null argument, or n_tris outside [0, 2^31 - 1]"); return ADYPT_E_INVALID; }
	const uint8_t *a = (const uint8_t *)rest, *b = (const uint8_t *)target;
	int64_t count = 0;
	for(int64_t i = 0; i < n_tris; ++i)
	{
		float r[kMorphWords], t[kMorphWords];
		memcpy(r, a + i * sizeof(TriRec), sizeof(r));
		memcpy(t, b + i * sizeof(TriRec), sizeof(t));
		if(!memcmp(r, t, sizeof(r))) continue;
		if(triangle_out) triangle_out[count] = (int32_t)i;
		if(deltas_out)
			for(int j = 0; j < kMorphWords; ++j) deltas_out[count * kMorphWords + j] = t[j] - r[j];
		++count;
	}
	return count;
}
