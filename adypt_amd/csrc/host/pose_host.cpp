// adypt_pose_triangles (include/adypt_host.h): triangles posed by part or joint matrices, on the host.  The rule is ../device/pose.hpp — the text the
// device path (pose.hip, k_pose) compiles too.
#include "common.hpp"
#include "../device/pose.hpp"
#include "../../../include/adypt_hip.h"
#include "../../../include/adypt_host.h"

using namespace adypt;

int adypt_pose_triangles(const void *triangles_in, int64_t n_tris, const int32_t *parts, const uint16_t *joints, const float *weights, const float *matrices, int32_t n_matrices,
                         void *triangles_out)
{
	const std::string who = "adypt_pose_triangles: ";
	const bool by_parts = parts != nullptr;
	if(n_tris < 0) { set_host_error(who + "n_tris is negative"); return ADYPT_E_INVALID; }
	if(!triangles_in || !triangles_out || !matrices) { set_host_error(who + "null argument"); return ADYPT_E_INVALID; }
	if(by_parts ? (joints || weights) : (!joints || !weights)) { set_host_error(who + "give either parts, or joints and weights"); return ADYPT_E_INVALID; }
	const char *why = pose_refuse_count(n_matrices);
	if(!why) why = by_parts ? pose_refuse_parts(parts, n_tris, n_matrices) : pose_refuse_skin(joints, weights, n_tris, n_matrices);
	if(!why) why = pose_refuse_matrices(matrices, n_matrices);
	if(why) { set_host_error(who + why); return ADYPT_E_INVALID; }
	const uint8_t *in = (const uint8_t *)triangles_in;
	uint8_t *out = (uint8_t *)triangles_out;
	for(int64_t i = 0; i < n_tris; ++i)
	{
		TriRec t;
		memcpy(&t, in + i * sizeof(TriRec), sizeof(TriRec));
		TriRec posed = t; // (texture coordinates and material id stay)
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
			const float p[3] = {t.p[v].x, t.p[v].y, t.p[v].z}, n[3] = {t.n[v].x, t.n[v].y, t.n[v].z};
			float p_out[3], n_out[3];
			pose_vertex(M, p, n, p_out, n_out);
			posed.p[v] = Vec3{p_out[0], p_out[1], p_out[2]};
			posed.n[v] = Vec3{n_out[0], n_out[1], n_out[2]};
		}
		memcpy(out + i * sizeof(TriRec), &posed, sizeof(TriRec));
	}
	return ADYPT_OK;
}
