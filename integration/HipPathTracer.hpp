// The reference-side binding of INTEGRATION.md as a real header: dropped into Adypt as src/Tracer/HipPathTracer.hpp (and
// linked with -ladypt_hip) it replaces OglScene + OglPathTracer behind the same method names.  It is written against the
// reference's own headers (Scene, WideBVH, InstanceConfig, tinyobj, stb_image, tinyexr, glm) and is syntax-checked against
// them by tests/test_integration_header.py whenever /root/reference is present; nothing of the reference is copied here.
//
//   Instance.hpp:   HipPathTracer m_path_tracer;                       // instead of OglScene m_oglscene; OglPathTracer m_path_tracer;
//   Instance.cpp:   m_path_tracer.Initialize(&m_config.m_pt_cfg, scene, wbvh, m_config.m_width, m_config.m_height);
//                   m_path_tracer.SetCamera(m_camera.GetProjection(), m_camera.GetView(), m_config.m_cam_cfg.m_position);
//                   m_path_tracer.Trace(enable_pt);  ...  m_path_tracer.SaveResult(name, fp16);
#ifndef ADYPT_HIPPATHTRACER_HPP
#define ADYPT_HIPPATHTRACER_HPP

#include <adypt_hip.h>

#include "../Util/Scene.hpp"
#include "../BVH/WideBVH.hpp"
#include "../InstanceConfig.hpp"

#include <glm/glm.hpp>
#include <stb_image.h>
#include <tinyexr.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

class HipPathTracer
{
public:
	enum ViewerTypes { kDiffuse = 0, kSpecular, kEmissive, kPTRadiance, kNormal, kPosition };
	ViewerTypes m_viewer_type = kDiffuse;

	// the 64-byte record uuMaterials holds (shaders/pathtracer.glsl:10-19): what SetMaterials takes
	struct GPUMaterial
	{
		int32_t m_dtex; float m_dr, m_dg, m_db;
		int32_t m_etex; float m_er, m_eg, m_eb;
		int32_t m_stex; float m_sr, m_sg, m_sb;
		int32_t m_illum; float m_shininess, m_dissolve, m_refraction_index;
	};
	static_assert(sizeof(GPUMaterial) == 64, "material record layout");

private:

	adypt_multi *m_gpus = nullptr; // one tile shard per device; a single device is the n_dev = 1 case of the same calls
	const InstanceConfig::PT *m_config = nullptr;
	int m_width = 0, m_height = 0;
	std::vector<GPUMaterial> m_materials;
	std::vector<adypt_texture> m_textures;
	std::vector<unsigned char *> m_texture_pixels; // stbi_load results, freed in the destructor

	// the end of SetMaterials, UpdateTexture and SetTriangleAttributes
	bool appearance_done(int code, adypt_appearance_info *info)
	{
		if(code == ADYPT_OK && (!info || adypt_get_appearance(adypt_multi_context(m_gpus, 0), info) == ADYPT_OK)) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// diffuse textures are shared by name; 8-bit RGB, first row = top (Scene.cpp flips v at load)
	int load_texture(std::map<std::string, int> &by_name, const std::string &filename)
	{
		std::map<std::string, int>::const_iterator it = by_name.find(filename);
		if(it != by_name.end()) return it->second;
		int w = 0, h = 0, channels = 0;
		unsigned char *data = stbi_load(filename.c_str(), &w, &h, &channels, 3);
		if(!data) { printf("[SCENE]ERR: unable to load texture %s\n", filename.c_str()); return -1; }
		adypt_texture t;
		t.width = w; t.height = h; t.rgb = data;
		m_textures.push_back(t);
		m_texture_pixels.push_back(data);
		return by_name[filename] = (int)m_textures.size() - 1;
	}

	void init_materials(const Scene &scene)
	{
		std::map<std::string, int> by_name;
		for(const tinyobj::material_t &ml : scene.GetTinyobjMaterials())
		{
			GPUMaterial g;
			g.m_dtex = ml.diffuse_texname.empty() ? -1 : load_texture(by_name, scene.GetBasePath() + ml.diffuse_texname);
			g.m_dr = ml.diffuse[0]; g.m_dg = ml.diffuse[1]; g.m_db = ml.diffuse[2];
			g.m_etex = -1; g.m_er = ml.emission[0]; g.m_eg = ml.emission[1]; g.m_eb = ml.emission[2];
			g.m_stex = -1; g.m_sr = ml.specular[0]; g.m_sg = ml.specular[1]; g.m_sb = ml.specular[2];
			g.m_illum = ml.illum; g.m_shininess = ml.shininess; g.m_dissolve = ml.dissolve; g.m_refraction_index = ml.ior;
			m_materials.push_back(g);
		}
	}

	bool update_config_args()
	{
		adypt_pt_params p;
		p.stack_size = m_config->m_stack_size; p.max_bounce = m_config->m_max_bounce;
		p.subpixel = m_config->m_subpixel; p.tmp_lifetime = m_config->m_tmp_lifetime;
		p.ray_tmin = m_config->m_ray_tmin; p.clamp = m_config->m_clamp;
		p.sun[0] = m_config->m_sun.x; p.sun[1] = m_config->m_sun.y; p.sun[2] = m_config->m_sun.z;
#ifdef ADYPT_BINDING_FIXED_SEED
		p.shift_seed = ADYPT_BINDING_FIXED_SEED; // reproducible runs (tests); the reference seeds its shift image from std::random_device
#else
		p.shift_seed = std::random_device{}();
#endif
		return adypt_multi_set_params(m_gpus, &p) == ADYPT_OK;
	}

	// PlanByHistory and TraceByHistory
	bool by_history(bool trace, int target, adypt_history_plan *out, std::vector<float> *reach, int minSpp, int maxSpp, int step, int tolerancePermille, float historyCap, bool followMotion,
	                bool moments)
	{
		const adypt_history_plan_params p = {target, minSpp, maxSpp, step, tolerancePermille, historyCap, followMotion ? 1 : 0, moments ? 1 : 0};
		if(trace && adypt_multi_get_spp(m_gpus) == 0) update_config_args(); // (a plan alone leaves everything to the call that traces)
		if(trace) m_viewer_type = kPTRadiance;
		if(reach) reach->resize((size_t)m_width * m_height);
		if((trace ? adypt_multi_trace_by_history(m_gpus, &p, out) : adypt_multi_plan_by_history(m_gpus, &p, out)) == ADYPT_OK &&
		   (!reach || adypt_multi_read_history_reach(m_gpus, reach->data()) == ADYPT_OK)) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

public:
	HipPathTracer() = default;
	HipPathTracer(const HipPathTracer &) = delete;
	HipPathTracer &operator=(const HipPathTracer &) = delete;
	~HipPathTracer()
	{
		adypt_destroy_multi(m_gpus);
		for(unsigned char *p : m_texture_pixels) stbi_image_free(p);
	}

	// OglScene::Initialize(scene, bvh) + OglPathTracer::Initialize(config, oglscene, width, height).
	// devices: HIP device ordinals; with more than one the frame is sharded by 32x32 pixel tile over them (scene replicated,
	// no communication while rendering) and SaveResult gathers the radiance on devices[0] over RCCL.
	// lookahead_frames: Instance::Update calls Trace(true) once per window frame.  0 (default, the windowed application): every call
	// traces exactly its one frame — even frame pacing, the smallest ray queues (1 frame in flight: ~0.4 GB per device at 1080p).
	// N > 0 (headless rendering, e.g. the CLI loop that calls Trace(true) spp times and then SaveResult): a call that needs an untraced
	// frame traces a whole wavefront pass of N frames and the following N - 1 calls only apply their running-mean step — 1.4x the
	// rays per second (DESIGN.md §4 "one frame per call"), but bursty: one call in N takes N frames' time, and the queues grow to
	// N frames in flight (8 x 16 B x N x pixels per device).  Images are bit-identical either way.
	// 1 (a good default for a window): still one frame per wavefront pass and the smallest queues, but the frame after the one asked for is STARTED on a
	// second HIP stream before the call returns (under the end of the current frame's launch: +15 % at 1080p, even pacing); it is dropped when the camera
	// moves, a viewer frame is traced or the sample counter is reset.
	bool Initialize(const InstanceConfig::PT *config, const Scene &scene, const WideBVH &bvh, int width, int height,
	                const std::vector<int> &devices = std::vector<int>(1, 0), int lookahead_frames = 0)
	{
		return create(config, scene, &bvh, width, height, devices, lookahead_frames, nullptr, 1, 8, 0.0, nullptr);
	}

private:
	// bvh null: no tree is uploaded; every device builds its first one from the triangles (adypt_create_multi_from_triangles)
	bool create(const InstanceConfig::PT *config, const Scene &scene, const WideBVH *bvh, int width, int height, const std::vector<int> &devices, int lookahead_frames,
	            const adypt_bvh_params *params, int method, int radius, double split_budget, adypt_rebuild_info *info)
	{
		m_config = config; m_width = width; m_height = height;
		init_materials(scene);
		adypt_scene_desc d;
		memset(&d, 0, sizeof(d));
		if(bvh)
		{
			d.nodes = bvh->GetNodes().data();            d.n_nodes = (int64_t)bvh->GetNodes().size();
			d.tri_indices = bvh->GetTriIndices().data(); d.n_refs = (int64_t)bvh->GetTriIndices().size();
		}
		d.woop = nullptr;                           // computed like OglScene::init_triangles
		d.triangles = scene.GetTriangles().data();  d.n_tris = (int64_t)scene.GetTriangles().size();
		d.materials = m_materials.data();           d.n_mats = (int64_t)m_materials.size();
		d.textures = m_textures.data();             d.n_textures = (int32_t)m_textures.size();
		d.width = width; d.height = height;
		const int made = bvh ? adypt_create_multi(&m_gpus, &d, devices.data(), (int)devices.size())
		                     : adypt_create_multi_from_triangles(&m_gpus, &d, devices.data(), (int)devices.size(), params, method, radius, split_budget, info);
		if(made != ADYPT_OK) { printf("[PT]ERR: %s\n", adypt_multi_last_error(nullptr)); return false; }
		const int fif = lookahead_frames > 0 ? (lookahead_frames < 128 ? lookahead_frames : 128) : 1;
		for(int i = 0; i < adypt_multi_device_count(m_gpus); ++i)
			if(adypt_set_frames_in_flight(adypt_multi_context(m_gpus, i), fif) != ADYPT_OK) { printf("[PT]ERR: %s\n", adypt_last_error(adypt_multi_context(m_gpus, i))); return false; }
		adypt_multi_set_lookahead(m_gpus, lookahead_frames > 0 ? 1 : 0);
		return update_config_args();
	}

public:

	void SetCamera(const glm::mat4 &projection, const glm::mat4 &view, const glm::vec3 &position)
	{
		const glm::mat4 inv_projection = glm::inverse(projection), inv_view = glm::inverse(view);
		adypt_multi_set_camera(m_gpus, &position.x, &inv_projection[0][0], &inv_view[0][0]);
	}

	// Trace(true): one more sample per pixel; Trace(false): one primary-ray viewer frame and the sample counter restarts
	void Trace(bool enable_pt)
	{
		if(enable_pt)
		{
			if(adypt_multi_get_spp(m_gpus) == 0) update_config_args(); // the config is re-read when path tracing (re)starts
			m_viewer_type = kPTRadiance;
			if(adypt_multi_trace_spp(m_gpus, 1) != ADYPT_OK) printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		}
		else
		{
			if(m_viewer_type == kPTRadiance) m_viewer_type = kDiffuse;
			if(adypt_multi_trace_primary(m_gpus, m_viewer_type) != ADYPT_OK) printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		}
	}

	int GetSPP() const { return adypt_multi_get_spp(m_gpus); }

	// Noise statistics (adypt_hip.h, adypt_set_noise_stats): how converged the image is, and tracing until it is converged enough.
	// Switch them on while the sample counter is 0 (after Initialize, or after a Trace(false)); the image itself never changes.
	bool SetNoiseStats(bool enabled) { return adypt_multi_set_noise_stats(m_gpus, enabled ? 1 : 0) == ADYPT_OK; }
	// mean_noise / worst_block / worst_index of the whole image after GetSPP() >= 2 samples
	bool GetNoise(adypt_noise *out) const { return adypt_multi_get_noise(m_gpus, out) == ADYPT_OK; }
	// Trace(true) in steps of check_every until the noisiest 32x32 block is at or below `target` (and min_spp samples are in), or max_spp is reached
	bool TraceUntil(double target, int min_spp, int max_spp, int check_every, adypt_noise *out = nullptr)
	{
		if(adypt_multi_get_spp(m_gpus) == 0) update_config_args();
		m_viewer_type = kPTRadiance;
		if(adypt_multi_trace_until(m_gpus, target, min_spp, max_spp, check_every, out) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}
	// Adaptive sampling: as TraceUntil, but every 32x32 block stops at the check at which ITS mean noise is at or below `target`; ends when every block
	// has stopped or at max_spp.  Stopped blocks stay so (later Trace(true) calls pass them over) until a Trace(false) or a reset of the accumulation.
	bool TraceAdaptive(double target, int min_spp, int max_spp, int check_every, adypt_adaptive *out = nullptr)
	{
		if(adypt_multi_get_spp(m_gpus) == 0) update_config_args();
		m_viewer_type = kPTRadiance;
		if(adypt_multi_trace_adaptive(m_gpus, target, min_spp, max_spp, check_every, out) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// History-aware sampling (adypt_hip.h, adypt_plan_by_history): before the first sample of a pose — a camera set, the counter at 0, the noise statistics
	// on — every 32x32 block gets the smallest sample count of minSpp, minSpp + step, ..., maxSpp that brings all but tolerancePermille / 1000 of its hit
	// pixels to `target` samples, the history DenoiseTemporal (followMotion: DenoiseTemporalMotion; moments: DenoiseTemporalMoments) will find for them and
	// their own together.  PlanByHistory only plans: nothing is traced or frozen, and no later call sees a difference.  TraceByHistory also traces: every
	// block holds the pixels of the uniform image at its own count afterwards.  reach (may be null): W x H floats, the samples of history every pixel
	// will find.  Not covered: DenoiseTemporalRectified (the plan may overestimate its history) and DenoiseTemporalSpecular.
	bool PlanByHistory(int target, adypt_history_plan *out = nullptr, std::vector<float> *reach = nullptr, int minSpp = 2, int maxSpp = 64, int step = 4, int tolerancePermille = 31,
	                   float historyCap = 64.0f, bool followMotion = false, bool moments = false)
	{
		return by_history(false, target, out, reach, minSpp, maxSpp, step, tolerancePermille, historyCap, followMotion, moments);
	}
	bool TraceByHistory(int target, adypt_history_plan *out = nullptr, std::vector<float> *reach = nullptr, int minSpp = 2, int maxSpp = 64, int step = 4, int tolerancePermille = 31,
	                    float historyCap = 64.0f, bool followMotion = false, bool moments = false)
	{
		return by_history(true, target, out, reach, minSpp, maxSpp, step, tolerancePermille, historyCap, followMotion, moments);
	}

	// Moving geometry (adypt_hip.h, adypt_update_triangles): new positions (count x 9 floats, p0 p1 p2 per triangle) and, unless null, normals (count x 9)
	// of triangles [first, first + count) in the order of Scene::GetTriangles(); every device then refits its BVH and Woop data on the GPU — no rebuild,
	// no new context.  The sample counter restarts as after a Trace(false).  A pose far from the one the BVH was built for traverses slower than a
	// rebuilt BVH would (Moving geometry).
	bool UpdateTriangles(int64_t first, int64_t count, const float *positions, const float *normals = nullptr)
	{
		if(adypt_multi_update_triangles(m_gpus, first, count, positions, normals) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// A new BVH for the triangles as UpdateTriangles left them, built on every device from its own copy (adypt_hip.h, adypt_rebuild_bvh): no upload, no new
	// context.  The SAH costs are the BVH section's of the config (nullptr: its defaults).  *info: sizes, the levels of the wide tree — what stackSize has
	// to cover — and the depth of the binary tree.  The sample counter restarts as after a Trace(false).
	// method Linear (the default): the linear tree, as ever.  PLOC: the binary tree is built by PLOC with search radius `radius`, 1 .. 32
	// (adypt_rebuild_bvh_ploc) — a tighter tree on meshes for a few times the build time (Rebuilding on the GPU).
	// split_budget, PLOC only, 0 .. 1: large triangles are split into several references first, at most split_budget * n more than triangles
	// (adypt_rebuild_bvh_ploc_split) — for scenes with large triangles among small ones; 0 (the default): no splits.
	enum class RebuildMethod { Linear, PLOC };
	static_assert((int)RebuildMethod::Linear == 0 && (int)RebuildMethod::PLOC == 1, "a RebuildMethod is the `method` of adypt_hip.h: 0 linear, 1 ploc");
	bool RebuildBVH(const adypt_bvh_params *params = nullptr, adypt_rebuild_info *info = nullptr, RebuildMethod method = RebuildMethod::Linear, int radius = 8, double split_budget = 0.0)
	{
		if(method != RebuildMethod::PLOC && split_budget != 0.0) { printf("[PT]ERR: RebuildBVH: split_budget needs RebuildMethod::PLOC\n"); return false; }
		const int code = method != RebuildMethod::PLOC ? adypt_multi_rebuild_bvh(m_gpus, params, info)
		                 : split_budget != 0.0         ? adypt_multi_rebuild_bvh_ploc_split(m_gpus, params, radius, split_budget, info)
		                                               : adypt_multi_rebuild_bvh_ploc(m_gpus, params, radius, info);
		if(code == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// Initialize without a WideBVH: no tree is built on the host and none is uploaded; every device builds its first tree from the triangles, as
	// RebuildBVH(params, info, method, radius, split_budget) would (adypt_hip.h, adypt_create_from_triangles) — milliseconds instead of the SBVH builder's
	// seconds, for a tree that traverses somewhat slower (Rebuilding on the GPU).
	bool Initialize(const InstanceConfig::PT *config, const Scene &scene, int width, int height, const std::vector<int> &devices = std::vector<int>(1, 0),
	                int lookahead_frames = 0, const adypt_bvh_params *params = nullptr, RebuildMethod method = RebuildMethod::PLOC, int radius = 8, double split_budget = 0.0,
	                adypt_rebuild_info *info = nullptr)
	{
		return create(config, scene, nullptr, width, height, devices, lookahead_frames, params, (int)method, radius, split_budget, info);
	}

	// Other triangles, any number of them (adypt_hip.h, adypt_set_triangles): every device packs them and builds their tree on the GPU as
	// RebuildBVH(params, info, method, radius, split_budget) would; materials, textures, camera and config stay, no new context.  Nothing changes when it
	// fails.  The sample counter restarts as after a Trace(false).
	bool SetTriangles(const std::vector<Triangle> &triangles, const adypt_bvh_params *params = nullptr, adypt_rebuild_info *info = nullptr,
	                  RebuildMethod method = RebuildMethod::PLOC, int radius = 8, double split_budget = 0.0)
	{
		static_assert(sizeof(Triangle) == 100, "Triangle is the 100-byte record adypt_set_triangles takes");
		if(adypt_multi_set_triangles(m_gpus, triangles.data(), (int64_t)triangles.size(), params, (int)method, radius, split_budget, info) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// The SAH cost of the tree the devices hold now, measured there from the quantised boxes (adypt_hip.h, adypt_get_tree_cost): what a refitted tree's
	// traversal work is proportional to.  params: the BVH section's SAH costs (nullptr: its defaults).
	bool GetTreeCost(adypt_tree_cost *cost, const adypt_bvh_params *params = nullptr)
	{
		if(adypt_multi_get_tree_cost(m_gpus, params, cost) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// UpdateTriangles that decides about a rebuild itself (adypt_hip.h, adypt_update_triangles_auto): after the refit the tree's cost is measured, and where
	// it is above policy.rebuild_above times the cost the tree had as uploaded or as last rebuilt, the tree is rebuilt as RebuildBVH(params, ..., method,
	// radius, split_budget) would.  rebuild_above has no default: see DESIGN.md, Moving geometry, for how to choose it.  *outcome (may be nullptr): the
	// three costs, whether the rebuild ran, and its info.
	struct PosePolicy
	{
		double rebuild_above;
		RebuildMethod method;
		int radius;
		double split_budget;
		explicit PosePolicy(double above, RebuildMethod m = RebuildMethod::PLOC, int r = 8, double budget = 0.0) : rebuild_above(above), method(m), radius(r), split_budget(budget) {}
		adypt_pose_policy abi() const { return adypt_pose_policy{rebuild_above, (int)method, radius, split_budget}; }
	};
	bool UpdateTriangles(int64_t first, int64_t count, const float *positions, const float *normals, const PosePolicy &policy, adypt_pose_outcome *outcome = nullptr,
	                     const adypt_bvh_params *params = nullptr)
	{
		const adypt_pose_policy p = policy.abi();
		if(adypt_multi_update_triangles_auto(m_gpus, first, count, positions, normals, params, &p, outcome) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// Posing on the GPU (adypt_hip.h, adypt_bind_parts / adypt_bind_skin / adypt_pose): bind once, then move the scene by 3x4 matrices — only the
	// matrices cross the bus.  BindParts: one part per triangle of Scene::GetTriangles(), 0 <= part < n_parts.  BindSkin: four weighted joints per
	// vertex (triangles x 12 each: vertex v's slots at 4 v; a slot of weight 0 is skipped).  Either makes every device keep the triangles as they are
	// then as the rest pose, from which every Pose starts; a refused call leaves an earlier binding in place, SetTriangles drops it.
	bool BindParts(const std::vector<int32_t> &part_of_triangle, int32_t n_parts)
	{
		if(adypt_multi_bind_parts(m_gpus, part_of_triangle.data(), (int64_t)part_of_triangle.size(), n_parts) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}
	bool BindSkin(const std::vector<uint16_t> &joints, const std::vector<float> &weights, int32_t n_joints)
	{
		if(joints.size() != weights.size() || joints.size() % 12 != 0) { printf("[PT]ERR: BindSkin: joints and weights are 12 per triangle\n"); return false; }
		if(adypt_multi_bind_skin(m_gpus, joints.data(), weights.data(), (int64_t)(joints.size() / 12), n_joints) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}
	// matrices: one per part or joint, 12 floats each, row-major 3x4 ([r][0..2] linear, [r][3] translation; a glm::mat4x3 is its transpose).  The tree is
	// refitted as UpdateTriangles refits it; the sample counter restarts as after a Trace(false).
	bool Pose(const std::vector<float> &matrices)
	{
		if(matrices.size() % 12 == 0 && adypt_multi_pose(m_gpus, matrices.data(), (int32_t)(matrices.size() / 12), nullptr, nullptr, nullptr) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", matrices.size() % 12 ? "Pose: a matrix is 12 floats" : adypt_multi_last_error(m_gpus));
		return false;
	}
	// ... and decides about a rebuild itself, as the UpdateTriangles overload above does
	bool Pose(const std::vector<float> &matrices, const PosePolicy &policy, adypt_pose_outcome *outcome = nullptr, const adypt_bvh_params *params = nullptr)
	{
		const adypt_pose_policy p = policy.abi();
		if(matrices.size() % 12 == 0 && adypt_multi_pose(m_gpus, matrices.data(), (int32_t)(matrices.size() / 12), params, &p, outcome) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", matrices.size() % 12 ? "Pose: a matrix is 12 floats" : adypt_multi_last_error(m_gpus));
		return false;
	}
	bool UnbindPose() { return adypt_multi_unbind_pose(m_gpus) == ADYPT_OK; }

	// Morph targets (blend shapes) in front of the matrices (adypt_hip.h, adypt_bind_morph / adypt_pose_morph): BindMorph adds a layer of sparse
	// entries to the binding BindParts or BindSkin made (a figure without a skeleton binds one part and poses it with the identity).  Entry e moves
	// triangle triangle_of_entry[e] by deltas[18 e .. 18 e + 17] (the deltas of p0 p1 p2, then of n0 n1 n2) times the weight of target
	// target_of_entry[e]; entries in any order, one per (triangle, target) at most; adypt_morph_diff (adypt_host.h) makes them from a target mesh.  A
	// refused call leaves an earlier layer in place; BindParts, BindSkin, UnbindPose and SetTriangles drop the layer, UnbindMorph drops only it.
	bool BindMorph(const std::vector<int32_t> &triangle_of_entry, const std::vector<int32_t> &target_of_entry, const std::vector<float> &deltas, int32_t n_targets)
	{
		const bool shaped = triangle_of_entry.size() == target_of_entry.size() && deltas.size() == 18 * triangle_of_entry.size();
		if(shaped && adypt_multi_bind_morph(m_gpus, triangle_of_entry.data(), target_of_entry.data(), deltas.data(), (int64_t)triangle_of_entry.size(), n_targets) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", shaped ? adypt_multi_last_error(m_gpus) : "BindMorph: an entry is a triangle, a target and 18 deltas");
		return false;
	}
	bool UnbindMorph() { return adypt_multi_unbind_morph(m_gpus) == ADYPT_OK; }
	// Pose with one weight per target of the layer (finite, any sign): only the weights and the matrices cross the bus.  Pose(matrices) on a binding
	// with a layer is this with every weight 0.
	bool Pose(const std::vector<float> &matrices, const std::vector<float> &morph_weights)
	{
		if(matrices.size() % 12 == 0 &&
		   adypt_multi_pose_morph(m_gpus, matrices.data(), (int32_t)(matrices.size() / 12), morph_weights.data(), (int32_t)morph_weights.size(), nullptr, nullptr, nullptr) == ADYPT_OK)
			return true;
		printf("[PT]ERR: %s\n", matrices.size() % 12 ? "Pose: a matrix is 12 floats" : adypt_multi_last_error(m_gpus));
		return false;
	}
	bool Pose(const std::vector<float> &matrices, const std::vector<float> &morph_weights, const PosePolicy &policy, adypt_pose_outcome *outcome = nullptr,
	          const adypt_bvh_params *params = nullptr)
	{
		const adypt_pose_policy p = policy.abi();
		if(matrices.size() % 12 == 0 &&
		   adypt_multi_pose_morph(m_gpus, matrices.data(), (int32_t)(matrices.size() / 12), morph_weights.data(), (int32_t)morph_weights.size(), params, &p, outcome) == ADYPT_OK)
			return true;
		printf("[PT]ERR: %s\n", matrices.size() % 12 ? "Pose: a matrix is 12 floats" : adypt_multi_last_error(m_gpus));
		return false;
	}

	// Poses given by vertices (adypt_hip.h, adypt_bind_mesh / adypt_pose_vertices): for a mesh that neither matrices nor blend weights move — cloth, a
	// soft body, a vertex cache.  BindMesh gives every corner of Scene::GetTriangles() a vertex (three indices per triangle, each below n_vertices;
	// adypt_weld_triangles of adypt_host.h makes them from the soup); PoseVertices then uploads one position per vertex (3 floats) and, unless normals
	// is empty, one normal per vertex (used as given); with normals empty the device computes smooth normals itself.  The tree is refitted as
	// UpdateTriangles refits it.  Independent of BindParts / BindSkin: whoever wrote the records last stands.  A refused call leaves an earlier mesh
	// binding in place; SetTriangles drops it.
	bool BindMesh(const std::vector<int32_t> &indices, int64_t n_vertices)
	{
		if(indices.size() % 3 == 0 && adypt_multi_bind_mesh(m_gpus, indices.data(), (int64_t)(indices.size() / 3), n_vertices) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", indices.size() % 3 ? "BindMesh: indices are three per triangle" : adypt_multi_last_error(m_gpus));
		return false;
	}
	bool PoseVertices(const std::vector<float> &positions, const std::vector<float> &normals = std::vector<float>())
	{
		const bool shaped = positions.size() % 3 == 0 && (normals.empty() || normals.size() == positions.size());
		if(shaped && adypt_multi_pose_vertices(m_gpus, positions.data(), normals.empty() ? nullptr : normals.data(), (int64_t)(positions.size() / 3), nullptr, nullptr, nullptr) == ADYPT_OK)
			return true;
		printf("[PT]ERR: %s\n", shaped ? adypt_multi_last_error(m_gpus) : "PoseVertices: three floats per vertex, as many normals as positions or none");
		return false;
	}
	// ... and decides about a rebuild itself, as the UpdateTriangles overload above does
	bool PoseVertices(const std::vector<float> &positions, const std::vector<float> &normals, const PosePolicy &policy, adypt_pose_outcome *outcome = nullptr,
	                  const adypt_bvh_params *params = nullptr)
	{
		const adypt_pose_policy p = policy.abi();
		const bool shaped = positions.size() % 3 == 0 && (normals.empty() || normals.size() == positions.size());
		if(shaped && adypt_multi_pose_vertices(m_gpus, positions.data(), normals.empty() ? nullptr : normals.data(), (int64_t)(positions.size() / 3), params, &p, outcome) == ADYPT_OK)
			return true;
		printf("[PT]ERR: %s\n", shaped ? adypt_multi_last_error(m_gpus) : "PoseVertices: three floats per vertex, as many normals as positions or none");
		return false;
	}
	bool UnbindMesh() { return adypt_multi_unbind_mesh(m_gpus) == ADYPT_OK; }

	// What the surfaces look like, changed on the GPU without a new context (adypt_hip.h, adypt_set_materials / adypt_update_texture /
	// adypt_set_triangle_attributes): a lamp switched on, a colour that fades, a texture that scrolls, triangles given another material.  SetMaterials
	// replaces the material table (any number of entries) and, with a texture list, ALL textures (width x height x 3 bytes each, which only have to
	// live until the call returns); without one the textures stay.  UpdateTexture writes new texels into one texture in place: its own size.
	// SetTriangleAttributes gives the triangles from `first` on material ids and / or texture coordinates (6 floats per triangle); an empty vector
	// leaves that attribute alone.  Tree, bindings and the denoiser's history stay; nothing changes when a call fails.  The sample counter restarts as
	// after UpdateTriangles.  *info (may be nullptr): the first device's counts, the triangles whose class changed, and the stage times.
	bool SetMaterials(const std::vector<GPUMaterial> &materials, adypt_appearance_info *info = nullptr)
	{
		static_assert(sizeof(GPUMaterial) == 64, "GPUMaterial is the 64-byte record adypt_set_materials takes");
		return appearance_done(adypt_multi_set_materials(m_gpus, materials.data(), (int64_t)materials.size(), nullptr, -1), info);
	}
	bool SetMaterials(const std::vector<GPUMaterial> &materials, const std::vector<adypt_texture> &textures, adypt_appearance_info *info = nullptr)
	{
		return appearance_done(adypt_multi_set_materials(m_gpus, materials.data(), (int64_t)materials.size(), textures.data(), (int32_t)textures.size()), info);
	}
	bool UpdateTexture(int32_t index, const uint8_t *rgb, int32_t width, int32_t height, adypt_appearance_info *info = nullptr)
	{
		return appearance_done(adypt_multi_update_texture(m_gpus, index, rgb, width, height), info);
	}
	bool SetTriangleAttributes(int64_t first, const std::vector<int32_t> &material_ids, const std::vector<float> &texcoords = std::vector<float>(), adypt_appearance_info *info = nullptr)
	{
		const bool shaped = texcoords.size() % 6 == 0 && (material_ids.empty() || texcoords.empty() || texcoords.size() == 6 * material_ids.size());
		if(!shaped) { printf("[PT]ERR: SetTriangleAttributes: six texture coordinates per triangle, as many triangles as material ids\n"); return false; }
		const int64_t count = (int64_t)(material_ids.empty() ? texcoords.size() / 6 : material_ids.size());
		return appearance_done(adypt_multi_set_triangle_attributes(m_gpus, first, count, material_ids.empty() ? nullptr : material_ids.data(), texcoords.empty() ? nullptr : texcoords.data()), info);
	}

	// The image through the denoiser with its history across poses (adypt_hip.h, adypt_denoise_temporal): W x H x 3 floats into *rgb.  Needs
	// SetNoiseStats(true) and GetSPP() >= 2.  commit: this call's state becomes the history (once per pose: after tracing, before the camera or the
	// scene changes).  followMotion (adypt_denoise_temporal_motion): a committing call also keeps every triangle's positions and normals, and a later
	// call merges a pixel on a triangle that UpdateTriangles or Pose has moved since through the point its hit had then — give it to every call of an
	// animation; SetTriangles and a committing call without it start the moved figure again.  params: levels and sigmas (nullptr: the defaults).
	bool DenoiseTemporal(std::vector<float> *rgb, float historyCap = 64.0f, bool commit = true, bool followMotion = false, const adypt_denoise_params *params = nullptr)
	{
		const adypt_temporal_params t = {historyCap, commit ? 1 : 0};
		rgb->resize((size_t)m_width * m_height * 3);
		if((followMotion ? adypt_multi_denoise_temporal_motion(m_gpus, params, &t) : adypt_multi_denoise_temporal(m_gpus, params, &t)) == ADYPT_OK &&
		   adypt_multi_read_denoised(m_gpus, rgb->data()) == ADYPT_OK) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// DenoiseTemporal with the history rectified (adypt_hip.h, adypt_denoise_temporal_rectified): before it is merged, the history is held against the
	// mean of the (2 radius + 1)^2 window of this call's own image on the pixel's surface, clamped to within gamma standard deviations of it, and loses
	// length by as much as it disagrees — for light that changed on a surface that stands still (a shadow that wandered, a door that opened).  radius
	// in [1, 3], gamma a finite number >= 0.  kept, where not null: W x H floats, the share of its length every pixel's history kept.
	bool DenoiseTemporalRectified(std::vector<float> *rgb, float historyCap = 64.0f, bool commit = true, bool followMotion = false, int radius = 3, float gamma = 1.0f,
	                              std::vector<float> *kept = nullptr, const adypt_denoise_params *params = nullptr)
	{
		const adypt_temporal_params t = {historyCap, commit ? 1 : 0};
		const adypt_rectify_params r = {radius, gamma};
		rgb->resize((size_t)m_width * m_height * 3);
		if(kept) kept->resize((size_t)m_width * m_height);
		if(adypt_multi_denoise_temporal_rectified(m_gpus, params, &t, &r, followMotion ? 1 : 0) == ADYPT_OK && adypt_multi_read_denoised(m_gpus, rgb->data()) == ADYPT_OK &&
		   (!kept || adypt_multi_read_denoise_rectify(m_gpus, kept->data()) == ADYPT_OK)) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// DenoiseTemporal from 1 spp per pose (adypt_hip.h, adypt_denoise_temporal_moments): needs GetSPP() >= 1.  The history carries the second moment of
	// the demodulated luminance, and the variance the filter sees is made after the merge — from the moments where the merged history is at least 4
	// samples long, from a 7 x 7 window on the pixel's surface where it is shorter.  Such a call and DenoiseTemporal do not find each other's history.
	// variance, where not null: W x H floats, the variance the first level saw.  No rectified form and none with followed guides.
	bool DenoiseTemporalMoments(std::vector<float> *rgb, float historyCap = 64.0f, bool commit = true, bool followMotion = false, std::vector<float> *variance = nullptr,
	                            const adypt_denoise_params *params = nullptr)
	{
		const adypt_temporal_params t = {historyCap, commit ? 1 : 0};
		rgb->resize((size_t)m_width * m_height * 3);
		if(variance) variance->resize((size_t)m_width * m_height);
		if(adypt_multi_denoise_temporal_moments(m_gpus, params, &t, followMotion ? 1 : 0) == ADYPT_OK && adypt_multi_read_denoised(m_gpus, rgb->data()) == ADYPT_OK &&
		   (!variance || adypt_multi_read_denoise_variance(m_gpus, variance->data()) == ADYPT_OK)) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// The image through the denoiser with guides that follow perfect mirrors and glass (adypt_hip.h, adypt_denoise_specular): a pixel whose primary
	// hit is a delta material is guided by the first surface its chain of up to `bounces` reflections / transmissions (1 .. 8) ends on, and pixels of
	// different chain classes do not pool.  chain, where not null: W x H class codes (0 a primary miss, 1 a primary hit followed nowhere, 1 + L ended on a
	// surface after L bounces, -(L + 1) left the scene).  Over time: DenoiseTemporalSpecular.
	bool DenoiseSpecular(std::vector<float> *rgb, int bounces = 4, std::vector<int8_t> *chain = nullptr, const adypt_denoise_params *params = nullptr)
	{
		const adypt_specular_params s = {bounces};
		rgb->resize((size_t)m_width * m_height * 3);
		if(chain) chain->resize((size_t)m_width * m_height);
		if(adypt_multi_denoise_specular(m_gpus, params, &s) == ADYPT_OK && adypt_multi_read_denoised(m_gpus, rgb->data()) == ADYPT_OK &&
		   (!chain || adypt_multi_read_denoise_guides_specular(m_gpus, bounces, nullptr, nullptr, nullptr, chain->data()) == ADYPT_OK)) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// DenoiseTemporal through mirrors and glass (adypt_hip.h, adypt_denoise_temporal_specular): the guides of DenoiseSpecular(bounces), and a pixel whose
	// chain ended on a surface finds its history through its virtual point — the camera ray unfolded to the chain's full length, of a planar mirror the
	// mirror image of what it shows — with every tap held against the followed guides and the pixel's class.  Such a call finds only a history a call
	// with the same bounces left, and the other temporal calls none in its.  virtualPosition, where not null: W x H x 3 floats, the virtual point of every
	// followed pixel (the position guide of every other).  No followMotion, rectified or moments form.
	bool DenoiseTemporalSpecular(std::vector<float> *rgb, int bounces = 4, float historyCap = 64.0f, bool commit = true, std::vector<float> *virtualPosition = nullptr,
	                             const adypt_denoise_params *params = nullptr)
	{
		const adypt_temporal_params t = {historyCap, commit ? 1 : 0};
		const adypt_specular_params s = {bounces};
		rgb->resize((size_t)m_width * m_height * 3);
		if(virtualPosition) virtualPosition->resize((size_t)m_width * m_height * 3);
		if(adypt_multi_denoise_temporal_specular(m_gpus, params, &t, &s) == ADYPT_OK && adypt_multi_read_denoised(m_gpus, rgb->data()) == ADYPT_OK &&
		   (!virtualPosition || adypt_multi_read_denoise_virtual(m_gpus, virtualPosition->data(), nullptr) == ADYPT_OK)) return true;
		printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus));
		return false;
	}

	// what DrawScreen puts on screen, for a caller-owned W x H RGBA8 texture / window (every device fills in its own tiles)
	bool ReadScreen(std::vector<uint8_t> *rgba8) const
	{
		rgba8->resize((size_t)m_width * m_height * 4);
		if(adypt_multi_read_display(m_gpus, rgba8->data()) != ADYPT_OK) return false; // every device converts and writes its own tiles
		return true;
	}

	void SaveResult(const char *filename, bool save_as_fp16)
	{
		std::vector<float> pixels((size_t)m_width * m_height * 3);
		if(adypt_multi_read_radiance(m_gpus, pixels.data()) != ADYPT_OK) { printf("[PT]ERR: %s\n", adypt_multi_last_error(m_gpus)); return; }
		const char *err = nullptr;
		if(SaveEXR(pixels.data(), m_width, m_height, 3, save_as_fp16, filename, &err) < 0)
		{
			printf("[PT]ERR: %s\n", err);
			FreeEXRErrorMessage(err);
		}
		else printf("[PT]INFO: Saved image to %s\n", filename);
	}
};

#endif // ADYPT_HIPPATHTRACER_HPP
