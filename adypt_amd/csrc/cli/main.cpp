// adypt_hip — headless equivalent of the reference application for one .config file:
//   Instance::InitializeFromFile / Initialize (src/Instance.cpp:10-42,59-69) -> N x Trace(true) -> SaveResult
//   (src/Tracer/OglPathTracer.cpp:199-212).  The interactive window / ImGui front-end is out of scope.
// Three layers: parse_options (argv -> Options), check_options (what does not go together; what follows from the rest) — both in options.cpp, which
// holds the synopsis (USAGE) and describes every option — and main() below: named steps over one Session, each false for exit 1.
#include "adypt_hip.h"
#include "adypt_host.h"
#include "options.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct Session
{
	Options opt;
	adypt_config cfg;
	std::vector<adypt_config> history_cfg; // --history-from: the earlier poses, of which only the cameras are used
	adypt_scene *scene = nullptr;
	const void *tris = nullptr, *mats = nullptr, *tex = nullptr;
	int64_t n_tris = 0, n_mats = 0;
	int32_t n_tex = 0;
	adypt_scene *appearance = nullptr; // --materials-from: the scene whose material table and textures the context is given before the main render
	adypt_bvh *bvh = nullptr;
	adypt_multi *multi = nullptr;
	std::vector<float> pose_positions, pose_normals; // --pose: what replaces the scene's vertices and normals once the context exists
	std::vector<int32_t> mesh_indices;               // --by-vertices: the scene as loaded, welded; pose_positions and pose_normals are then per vertex
	int64_t n_vertices = 0;
	std::vector<int32_t> part_of_triangle;           // --part-matrices: the binding and one matrix per part, the identity where FILE names none
	std::vector<float> part_matrix;
	int32_t n_parts = 0;
	std::vector<int32_t> morph_triangle, morph_target; // --morph-target: the entries of all targets, each diffed against the scene as loaded
	std::vector<float> morph_deltas;
	adypt_pt_params params;
	float inv_proj[16], inv_view[16]; // the main config's camera
	adypt_denoise_params denoise_params;
	adypt_temporal_params temporal_params;
	std::vector<float> rgb;
	std::vector<uint8_t> rgba8;
	adypt_noise noise;
	adypt_adaptive adapt;
	adypt_history_plan plan;
	double render_ms = 0.0; // wall time of the render without its progressive saves
};

static double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- the two ways a step fails ----
static bool tracer_failed(const adypt_multi *multi, const char *before = "")
{
	fprintf(stderr, "%s[TRACER]Err: %s\n", before, adypt_multi_last_error(multi));
	return false;
}
static bool host_failed()
{
	fprintf(stderr, "[PT]ERR: %s\n", adypt_host_last_error());
	return false;
}

// ---- load the inputs: everything that can be wrong with files is found before a device is asked for ----
static bool load_configs(Session &s)
{
	const Options &o = s.opt;
	adypt_config &cfg = s.cfg;
	adypt_config_default(&cfg);
	if(adypt_config_load(o.config.c_str(), &cfg) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Invalid instance %s: %s\n", o.config.c_str(), adypt_host_last_error()); return false; }
	printf("[INSTANCE]Info: Instance loaded from %s\n", o.config.c_str());
	s.history_cfg.resize(o.history_from.size());
	for(size_t k = 0; k < o.history_from.size(); ++k)
	{
		adypt_config &h = s.history_cfg[k];
		adypt_config_default(&h);
		if(adypt_config_load(o.history_from[k].c_str(), &h) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Invalid instance %s: %s\n", o.history_from[k].c_str(), adypt_host_last_error()); return false; }
		if(strcmp(h.obj_filename, cfg.obj_filename) != 0 || h.width != cfg.width || h.height != cfg.height)
		{
			fprintf(stderr, "[INSTANCE]Err: --history-from %s names another scene or another size than %s (%s, %d x %d)\n", o.history_from[k].c_str(), o.config.c_str(), cfg.obj_filename, cfg.width, cfg.height);
			return false;
		}
	}
	return true;
}

static bool load_scene(Session &s)
{
	if(adypt_scene_load(s.cfg.obj_filename, &s.scene) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Unable to load scene %s: %s\n", s.cfg.obj_filename, adypt_host_last_error()); return false; }
	s.n_tris = adypt_scene_triangles(s.scene, &s.tris);
	s.n_mats = adypt_scene_materials(s.scene, &s.mats);
	s.n_tex = adypt_scene_textures(s.scene, &s.tex);
	printf("[SCENE]Info: %lld triangles loaded from %s\n", (long long)s.n_tris, s.cfg.obj_filename);
	if(*adypt_scene_warnings(s.scene)) printf("[SCENE]Warn: %s", adypt_scene_warnings(s.scene)); // undecodable textures: their materials render black
	return true;
}

// --by-vertices: the scene as loaded welded into an indexed mesh, and the pose's corners gathered into one position and one normal per vertex — those
// of the corner at which the vertex first appeared in the weld.  A pose that gives another corner of a vertex other position bits tears it: refused.
static bool pose_by_vertices(Session &s)
{
	s.mesh_indices.resize((size_t)s.n_tris * 3);
	s.n_vertices = adypt_weld_triangles(s.tris, s.n_tris, s.mesh_indices.data(), nullptr, nullptr);
	if(s.n_vertices < 0) return host_failed();
	std::vector<float> positions((size_t)s.n_vertices * 3), normals((size_t)s.n_vertices * 3);
	int64_t seen = 0; // (vertices are numbered in order of first appearance)
	for(int64_t corner = 0; corner < s.n_tris * 3; ++corner)
	{
		const int64_t v = s.mesh_indices[(size_t)corner];
		const size_t at = (size_t)(corner / 3) * 9 + (size_t)(corner % 3) * 3;
		if(v == seen)
		{
			memcpy(&positions[(size_t)v * 3], &s.pose_positions[at], 12);
			memcpy(&normals[(size_t)v * 3], &s.pose_normals[at], 12);
			++seen;
		}
		else if(memcmp(&positions[(size_t)v * 3], &s.pose_positions[at], 12) != 0)
		{
			fprintf(stderr, "[INSTANCE]Err: pose %s tears vertex %lld, which the scene shares: corner %lld of triangle %lld has another position than its first corner\n", s.opt.pose.c_str(), (long long)v,
			        (long long)(corner % 3), (long long)(corner / 3));
			return false;
		}
	}
	s.pose_positions.swap(positions);
	s.pose_normals.swap(normals);
	return true;
}

static bool load_pose(Session &s)
{
	const std::string &pose = s.opt.pose;
	if(pose.empty()) return true;
	adypt_scene *moved = nullptr;
	if(adypt_scene_load(pose.c_str(), &moved) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Unable to load pose %s: %s\n", pose.c_str(), adypt_host_last_error()); return false; }
	const void *mt;
	const int64_t n_moved = adypt_scene_triangles(moved, &mt);
	if(n_moved != s.n_tris) { fprintf(stderr, "[INSTANCE]Err: pose %s has %lld triangles, the scene has %lld\n", pose.c_str(), (long long)n_moved, (long long)s.n_tris); return false; }
	s.pose_positions.resize((size_t)s.n_tris * 9);
	s.pose_normals.resize((size_t)s.n_tris * 9);
	for(int64_t i = 0; i < s.n_tris; ++i) // (100-byte records: 9 position floats, 9 normal floats, ...)
	{
		memcpy(&s.pose_positions[(size_t)i * 9], (const uint8_t *)mt + i * 100, 36);
		memcpy(&s.pose_normals[(size_t)i * 9], (const uint8_t *)mt + i * 100 + 36, 36);
	}
	adypt_scene_free(moved);
	return !s.opt.by_vertices || pose_by_vertices(s);
}

// parts by material id, every matrix the identity but those the table of --part-matrices names
static bool load_parts(Session &s)
{
	const std::string &table = s.opt.part_matrices;
	if(table.empty() && !s.opt.morphing) return true;
	s.part_of_triangle.resize((size_t)s.n_tris);
	bool loose = false;
	for(int64_t i = 0; i < s.n_tris; ++i) // (100-byte records: the material id is the last word)
	{
		int32_t matid;
		memcpy(&matid, (const uint8_t *)s.tris + i * 100 + 96, 4);
		const bool known = matid >= 0 && matid < s.n_mats;
		s.part_of_triangle[(size_t)i] = known ? matid : (int32_t)s.n_mats;
		loose |= !known;
	}
	s.n_parts = (int32_t)s.n_mats + (loose ? 1 : 0);
	for(int32_t k = 0; k < s.n_parts; ++k)
		for(int j = 0; j < 12; ++j) s.part_matrix.push_back(j % 5 == 0 ? 1.0f : 0.0f);
	if(table.empty()) return true;
	FILE *f = fopen(table.c_str(), "r");
	if(!f) { fprintf(stderr, "[INSTANCE]Err: Unable to open %s\n", table.c_str()); return false; }
	char line[1024];
	for(int at = 1; fgets(line, sizeof(line), f); ++at)
	{
		if(char *hash = strchr(line, '#')) *hash = 0;
		long part;
		float m[12];
		int used = 0;
		const int got = sscanf(line, "%ld %f %f %f %f %f %f %f %f %f %f %f %f %n", &part, m, m + 1, m + 2, m + 3, m + 4, m + 5, m + 6, m + 7, m + 8, m + 9, m + 10, m + 11, &used);
		if(got <= 0 && line[strspn(line, " \t\r\n")] == 0) continue;
		if(got != 13 || line[used] != 0 || part < 0 || part >= s.n_parts)
		{
			fprintf(stderr, "[INSTANCE]Err: %s line %d is not `part m00 ... m23` with a part in [0, %d)\n", table.c_str(), at, (int)s.n_parts);
			fclose(f);
			return false;
		}
		memcpy(&s.part_matrix[(size_t)part * 12], m, sizeof(m));
	}
	fclose(f);
	return true;
}

static bool load_morph_targets(Session &s)
{
	for(size_t k = 0; k < s.opt.morph_targets.size(); ++k)
	{
		const char *path = s.opt.morph_targets[k].c_str();
		adypt_scene *target = nullptr;
		if(adypt_scene_load(path, &target) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Unable to load morph target %s: %s\n", path, adypt_host_last_error()); return false; }
		const void *tt;
		const int64_t n_target = adypt_scene_triangles(target, &tt);
		if(n_target != s.n_tris) { fprintf(stderr, "[INSTANCE]Err: morph target %s has %lld triangles, the scene has %lld\n", path, (long long)n_target, (long long)s.n_tris); return false; }
		const int64_t count = adypt_morph_diff(s.tris, tt, s.n_tris, nullptr, nullptr);
		if(count < 0) { fprintf(stderr, "[INSTANCE]Err: %s\n", adypt_host_last_error()); return false; }
		const size_t at = s.morph_triangle.size();
		s.morph_triangle.resize(at + (size_t)count);
		s.morph_deltas.resize((at + (size_t)count) * 18);
		s.morph_target.resize(at + (size_t)count, (int32_t)k);
		(void)adypt_morph_diff(s.tris, tt, s.n_tris, s.morph_triangle.data() + at, s.morph_deltas.data() + at * 18);
		adypt_scene_free(target);
	}
	return true;
}

static bool load_materials(Session &s)
{
	const std::string &other = s.opt.materials_from;
	if(other.empty()) return true;
	if(adypt_scene_load(other.c_str(), &s.appearance) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Unable to load materials %s: %s\n", other.c_str(), adypt_host_last_error()); return false; }
	if(*adypt_scene_warnings(s.appearance)) printf("[SCENE]Warn: %s", adypt_scene_warnings(s.appearance));
	return true;
}

// the cached .bvh, or a host build that is then cached; neither with --build gpu
static bool load_bvh(Session &s)
{
	adypt_config &cfg = s.cfg;
	if(s.opt.build_on_gpu || adypt_bvh_load(cfg.bvh_filename, &cfg.bvh, &s.bvh) == ADYPT_OK) return true;
	adypt_build_info info;
	if(adypt_bvh_build(s.scene, &cfg.bvh, &s.bvh, &info) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: bvh build failed: %s\n", adypt_host_last_error()); return false; }
	printf("[SBVH]building lasted %.0f ms, %lld nodes, %lld references\n[WideBVH]built with %lld nodes (%.0f ms)\n", info.sbvh_ms,
		   (long long)info.sbvh_nodes, (long long)info.refs, (long long)info.wide_nodes, info.wide_ms);
	if(adypt_bvh_save(s.bvh, cfg.bvh_filename, &cfg.bvh) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Unable to save bvh %s\n", cfg.bvh_filename); return false; }
	return true;
}

static bool load_inputs(Session &s)
{
	return load_configs(s) && load_scene(s) && load_pose(s) && load_parts(s) && load_morph_targets(s) && load_materials(s) && load_bvh(s);
}

// ---- the tracer ----
// the figures of a rebuild that has just run: what the rebuild line prints
static std::string rebuild_figures(const Session &s, const adypt_rebuild_info &info)
{
	const Options &o = s.opt;
	float ms[7] = {0, 0, 0, 0, 0, 0, 0};
	(void)adypt_get_rebuild_timing(adypt_multi_context(s.multi, 0), ms, 7);
	std::string method = o.ploc ? "ploc radius " + std::to_string(o.ploc_radius) : "linear";
	if(o.split_budget)
	{
		int32_t presplit[2] = {-1, 0};
		(void)adypt_get_rebuild_presplit(adypt_multi_context(s.multi, 0), presplit);
		char text[64];
		snprintf(text, sizeof(text), " split budget %g level %d", *o.split_budget, (int)presplit[0]);
		method += text;
	}
	char text[512];
	snprintf(text, sizeof(text), "%lld nodes, %lld references, %d levels, method %s, %.3f ms (keys %.3f, sort %.3f, tree %.3f, bottom-up %.3f, emission %.3f, Woop and nodes %.3f)", (long long)info.n_nodes,
	         (long long)info.n_refs, (int)info.levels, method.c_str(), ms[6], ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
	return std::string(text);
}

// any number of devices through the library's multi-device boundary (one device is its n_dev = 1 case): tile rank i on devices[i], one gather per saved image
static bool create_tracer(Session &s)
{
	const Options &o = s.opt;
	adypt_config &cfg = s.cfg;
	const void *nodes;
	const int32_t *idx;
	adypt_scene_desc d;
	memset(&d, 0, sizeof(d));
	if(s.bvh)
	{
		d.n_nodes = adypt_bvh_nodes(s.bvh, &nodes); d.nodes = nodes;
		d.n_refs = adypt_bvh_tri_indices(s.bvh, &idx); d.tri_indices = idx;
	}
	d.triangles = s.tris; d.n_tris = s.n_tris; d.materials = s.mats; d.n_mats = s.n_mats;
	d.textures = (const adypt_texture *)s.tex; d.n_textures = s.n_tex;
	d.width = cfg.width; d.height = cfg.height; d.device = o.devices[0]; d.tile_rank = 0; d.tile_nranks = 1;
	adypt_rebuild_info first_build;
	if((o.build_on_gpu ? adypt_create_multi_from_triangles(&s.multi, &d, o.devices.data(), (int)o.devices.size(), &cfg.bvh, o.policy.method, o.policy.radius, o.policy.split_budget, &first_build)
	                   : adypt_create_multi(&s.multi, &d, o.devices.data(), (int)o.devices.size())) != ADYPT_OK)
		return tracer_failed(nullptr);
	adypt_pt_params &p = s.params;
	p.stack_size = cfg.stack_size; p.max_bounce = cfg.max_bounce; p.subpixel = cfg.subpixel; p.tmp_lifetime = cfg.tmp_lifetime;
	p.ray_tmin = cfg.ray_tmin; p.clamp = cfg.clamp; memcpy(p.sun, cfg.sun, 12); p.shift_seed = o.seed;
	adypt_camera_matrices(cfg.fov, cfg.yaw, cfg.pitch, cfg.width, cfg.height, s.inv_proj, s.inv_view);
	int r = adypt_multi_set_params(s.multi, &p);
	if(r == ADYPT_OK) r = adypt_multi_set_camera(s.multi, cfg.position, s.inv_proj, s.inv_view);
	if(r == ADYPT_OK && o.sun_visibility) r = adypt_multi_set_sun_visibility(s.multi, 1, nullptr);
	if(r == ADYPT_OK) r = adypt_multi_set_instrumentation(s.multi, 1);
	if(r == ADYPT_OK && (o.until || o.denoise)) r = adypt_multi_set_noise_stats(s.multi, 1);
	if(r != ADYPT_OK) return tracer_failed(s.multi);
	if(o.build_on_gpu) printf("[PT]BUILD: %s\n", rebuild_figures(s, first_build).c_str());
	s.denoise_params = adypt_denoise_params{o.denoise_levels, 4.0f, 0.1f};
	s.temporal_params = adypt_temporal_params{(float)o.history_cap.value_or(64.0), 1};
	return true;
}

// what --rebuild-above made of a pose
static void print_pose_policy(const Session &s, const adypt_pose_outcome &outcome)
{
	if(!s.opt.rebuild_above) return;
	printf("[PT]INFO: pose policy: tree cost %.4f -> %.4f (ratio %.4f, allowed %g): %s\n", outcome.built.cost, outcome.refitted.cost, outcome.refitted.cost / outcome.built.cost, *s.opt.rebuild_above,
	       outcome.rebuilt ? ("rebuilt (" + rebuild_figures(s, outcome.rebuild) + ")").c_str() : "kept");
}

// --pose / --part-matrices / --morph-target and the rebuild that goes with them: before the history poses, or with --follow-motion after them
static bool move_scene(Session &s)
{
	const Options &o = s.opt;
	adypt_multi *multi = s.multi;
	adypt_config &cfg = s.cfg;
	const adypt_pose_policy *policy = o.rebuild_above ? &o.policy : nullptr;
	adypt_pose_outcome outcome;
	float ms[4] = {0, 0, 0, 0};
	if(o.by_vertices)
	{
		const float *normals = o.recompute_normals ? nullptr : s.pose_normals.data();
		adypt_mesh_binding mesh;
		memset(&mesh, 0, sizeof(mesh));
		int code = adypt_multi_bind_mesh(multi, s.mesh_indices.data(), s.n_tris, s.n_vertices);
		if(code == ADYPT_OK) code = adypt_multi_get_mesh_binding(multi, &mesh);
		if(code == ADYPT_OK) code = adypt_multi_pose_vertices(multi, s.pose_positions.data(), normals, s.n_vertices, &cfg.bvh, policy, &outcome);
		if(code != ADYPT_OK) return tracer_failed(multi);
		(void)adypt_get_refit_timing(adypt_multi_context(multi, 0), ms, 4);
		printf("[PT]MESH: vertices %lld triangles %lld max_valence %d normals %s\n", (long long)mesh.n_vertices, (long long)mesh.n_tris, (int)mesh.max_valence, normals ? "given" : "computed");
		printf("[PT]INFO: pose %s by vertices: refit %.3f ms (upload and mesh kernels %.3f, references and Woop %.3f, nodes %.3f)\n", o.pose.c_str(), ms[3], ms[0], ms[1], ms[2]);
		print_pose_policy(s, outcome);
	}
	else if(!o.pose.empty())
	{
		const int code = policy ? adypt_multi_update_triangles_auto(multi, 0, s.n_tris, s.pose_positions.data(), s.pose_normals.data(), &cfg.bvh, policy, &outcome)
		                        : adypt_multi_update_triangles(multi, 0, s.n_tris, s.pose_positions.data(), s.pose_normals.data());
		if(code != ADYPT_OK) return tracer_failed(multi);
		(void)adypt_get_refit_timing(adypt_multi_context(multi, 0), ms, 4);
		printf("[PT]INFO: pose %s: %lld triangles moved, refit %.3f ms (scatter %.3f, references and Woop %.3f, nodes %.3f)\n", o.pose.c_str(), (long long)s.n_tris, ms[3], ms[0], ms[1], ms[2]);
		print_pose_policy(s, outcome);
	}
	if(!o.part_matrices.empty() || o.morphing)
	{
		adypt_morph_binding layer;
		memset(&layer, 0, sizeof(layer));
		int code = adypt_multi_bind_parts(multi, s.part_of_triangle.data(), s.n_tris, s.n_parts);
		if(code == ADYPT_OK && o.morphing) code = adypt_multi_bind_morph(multi, s.morph_triangle.data(), s.morph_target.data(), s.morph_deltas.data(), (int64_t)s.morph_triangle.size(), (int32_t)o.morph_targets.size());
		if(code == ADYPT_OK && o.morphing) code = adypt_multi_get_morph_binding(multi, &layer);
		if(code == ADYPT_OK)
			code = o.morphing ? adypt_multi_pose_morph(multi, s.part_matrix.data(), s.n_parts, o.morph_weights.data(), (int32_t)o.morph_weights.size(), &cfg.bvh, policy, &outcome)
			                  : adypt_multi_pose(multi, s.part_matrix.data(), s.n_parts, &cfg.bvh, policy, &outcome);
		if(code != ADYPT_OK) return tracer_failed(multi);
		(void)adypt_get_refit_timing(adypt_multi_context(multi, 0), ms, 4);
		if(o.morphing) printf("[PT]MORPH: targets %d entries %lld triangles %lld of %lld\n", (int)layer.n_targets, (long long)layer.n_entries, (long long)layer.n_tris_touched, (long long)s.n_tris);
		if(o.part_matrices.empty()) printf("[PT]INFO: morph pose: refit %.3f ms (weights, matrices and pose %.3f, references and Woop %.3f, nodes %.3f)\n", ms[3], ms[0], ms[1], ms[2]);
		else printf("[PT]POSE: parts %d triangles %lld from %s, refit %.3f ms (matrices and pose %.3f, references and Woop %.3f, nodes %.3f)\n", (int)s.n_parts, (long long)s.n_tris, o.part_matrices.c_str(), ms[3],
		       ms[0], ms[1], ms[2]);
		print_pose_policy(s, outcome);
	}
	if(o.rebuild)
	{
		adypt_rebuild_info info;
		const int code = o.split_budget ? adypt_multi_rebuild_bvh_ploc_split(multi, &cfg.bvh, o.ploc_radius, *o.split_budget, &info)
		                 : o.ploc       ? adypt_multi_rebuild_bvh_ploc(multi, &cfg.bvh, o.ploc_radius, &info)
		                                : adypt_multi_rebuild_bvh(multi, &cfg.bvh, &info);
		if(code != ADYPT_OK) return tracer_failed(multi);
		printf("[PT]INFO: rebuild: %s\n", rebuild_figures(s, info).c_str());
	}
	return true;
}

// a temporal call as the options ask for it
static int temporal_call(Session &s)
{
	const Options &o = s.opt;
	const adypt_specular_params followed{o.follow_specular.value_or(0)};
	if(o.follow_specular) return adypt_multi_denoise_temporal_specular(s.multi, &s.denoise_params, &s.temporal_params, &followed);
	if(o.denoise_moments) return adypt_multi_denoise_temporal_moments(s.multi, &s.denoise_params, &s.temporal_params, o.follow_motion ? 1 : 0);
	if(o.rectify) return adypt_multi_denoise_temporal_rectified(s.multi, &s.denoise_params, &s.temporal_params, &o.rectify_params, o.follow_motion ? 1 : 0);
	return o.follow_motion ? adypt_multi_denoise_temporal_motion(s.multi, &s.denoise_params, &s.temporal_params) : adypt_multi_denoise_temporal(s.multi, &s.denoise_params, &s.temporal_params);
}

// --history-from: every earlier pose is rendered and committed to the denoiser's history, each with a shift_seed of its own (an unchanged seed would
// repeat the very same samples, which the history would count twice)
static bool commit_history_poses(Session &s)
{
	const Options &o = s.opt;
	for(size_t k = 0; k < s.history_cfg.size(); ++k)
	{
		const adypt_config &h = s.history_cfg[k];
		float hp[16], hv[16];
		adypt_camera_matrices(h.fov, h.yaw, h.pitch, s.cfg.width, s.cfg.height, hp, hv);
		s.params.shift_seed = o.seed + 1u + (unsigned)k;
		int r = adypt_multi_reset(s.multi);
		if(r == ADYPT_OK) r = adypt_multi_set_params(s.multi, &s.params);
		if(r == ADYPT_OK) r = adypt_multi_set_camera(s.multi, h.position, hp, hv);
		if(r == ADYPT_OK) r = adypt_multi_trace_spp(s.multi, o.spp);
		if(r == ADYPT_OK) r = temporal_call(s);
		if(r != ADYPT_OK) return tracer_failed(s.multi);
		printf("[PT]INFO: history pose %s: %d spp committed\n", o.history_from[k].c_str(), o.spp);
	}
	return true;
}

// --materials-from: after the history poses, which show the old surfaces, and before the main render
static bool swap_materials(Session &s)
{
	if(!s.appearance) return true;
	const void *mats, *tex;
	const int64_t n_mats = adypt_scene_materials(s.appearance, &mats);
	const int32_t n_tex = adypt_scene_textures(s.appearance, &tex);
	adypt_appearance_info info;
	if(adypt_multi_set_materials(s.multi, mats, n_mats, (const adypt_texture *)tex, n_tex) != ADYPT_OK || adypt_get_appearance(adypt_multi_context(s.multi, 0), &info) != ADYPT_OK)
		return tracer_failed(s.multi);
	printf("[PT]MATERIALS: materials %lld textures %d reclassed %lld of %lld triangles\n", (long long)info.n_mats, (int)info.n_textures, (long long)info.reclassed, (long long)s.n_tris);
	return true;
}

// after the history poses: the main config's camera and seed again, from 0 spp
static bool back_to_the_main_view(Session &s)
{
	if(s.history_cfg.empty()) return true;
	s.params.shift_seed = s.opt.seed;
	int r = adypt_multi_reset(s.multi);
	if(r == ADYPT_OK) r = adypt_multi_set_params(s.multi, &s.params);
	if(r == ADYPT_OK) r = adypt_multi_set_camera(s.multi, s.cfg.position, s.inv_proj, s.inv_view);
	return r == ADYPT_OK || tracer_failed(s.multi);
}

// ---- render ----
// SaveResult (OglPathTracer.cpp:199-212) + the window's picture; written to a temporary name first so that a reader of a
// progressive render never sees a half-written file
static bool save(Session &s)
{
	const Options &o = s.opt;
	const int w = s.cfg.width, h = s.cfg.height;
	s.rgb.assign((size_t)w * h * 3, 0.0f);
	if(adypt_multi_read_radiance(s.multi, s.rgb.data()) != ADYPT_OK) return tracer_failed(s.multi);
	const std::string tmp = o.out + ".part";
	if(adypt_save_exr(tmp.c_str(), s.rgb.data(), w, h, o.fp16) != ADYPT_OK || rename(tmp.c_str(), o.out.c_str()) != 0) return host_failed();
	if(!o.preview.empty())
	{
		s.rgba8.assign((size_t)w * h * 4, 0);
		if(adypt_multi_read_display(s.multi, s.rgba8.data()) != ADYPT_OK) return tracer_failed(s.multi);
		const std::string ptmp = o.preview + ".part";
		if(adypt_save_png(ptmp.c_str(), s.rgba8.data(), w, h) != ADYPT_OK || rename(ptmp.c_str(), o.preview.c_str()) != 0) return host_failed();
	}
	return true;
}

// a progressive save; its time does not count as the render's
static bool save_progress(Session &s, int spp, double *t_save)
{
	const double ts = now_ms();
	if(!save(s)) return false;
	*t_save += now_ms() - ts;
	printf("[PT]INFO: %d spp saved to %s\n", spp, s.opt.out.c_str());
	fflush(stdout);
	return true;
}

static bool render(Session &s)
{
	const Options &o = s.opt;
	adypt_multi *multi = s.multi;
	const double t0 = now_ms();
	double t_save = 0.0;
	int r = ADYPT_OK;
	memset(&s.noise, 0, sizeof(s.noise));
	memset(&s.adapt, 0, sizeof(s.adapt));
	memset(&s.plan, 0, sizeof(s.plan));
	if(o.history_samples)
	{
		// by the history: --spp is the cap, every block stops where history and own samples together reach the target
		const adypt_history_plan_params by_history{*o.history_samples, 2, o.spp, o.history_step, o.history_tolerance, s.temporal_params.history_cap, o.follow_motion ? 1 : 0, o.denoise_moments ? 1 : 0};
		r = adypt_multi_trace_by_history(multi, &by_history, &s.plan);
	}
	else if(o.adaptive)
	{
		r = adypt_multi_trace_adaptive(multi, o.noise_target, o.min_spp, o.spp, o.check_every, &s.adapt);
		s.noise = s.adapt.noise;
	}
	else if(o.until)
	{
		// to the noise target, --spp the cap.  With --save-every K the image is written whenever K more samples are in: the call is then capped at
		// the next multiple of K and taken up again (the noise is looked at every check_every samples from there).
		for(bool done = false; !done;)
		{
			const int now = adypt_multi_get_spp(multi);
			const int cap = o.save_every > 0 ? std::min(o.spp, std::max(2, (now / o.save_every + 1) * o.save_every)) : o.spp;
			r = adypt_multi_trace_until(multi, o.noise_target, std::min(o.min_spp, cap), cap, o.check_every, &s.noise);
			if(r != ADYPT_OK) break;
			done = s.noise.spp >= o.spp || (s.noise.spp >= o.min_spp && s.noise.worst_block <= o.noise_target);
			if(!done && !save_progress(s, s.noise.spp, &t_save)) return false;
		}
	}
	else if(o.primary >= 0) r = adypt_multi_trace_primary(multi, o.primary);
	else if(o.save_every <= 0 || o.save_every >= o.spp) r = adypt_multi_trace_spp(multi, o.spp);
	else
		for(int done = 0; done < o.spp && r == ADYPT_OK;)
		{
			const int n = std::min(o.save_every, o.spp - done);
			r = adypt_multi_trace_spp(multi, n);
			done += n;
			if(r == ADYPT_OK && done < o.spp && !save_progress(s, done, &t_save)) return false;
		}
	s.render_ms = now_ms() - t_save - t0;
	return r == ADYPT_OK || tracer_failed(multi);
}

// ---- report and save ----
static bool report_and_save_image(Session &s)
{
	const Options &o = s.opt;
	adypt_stats st;
	if(adypt_multi_get_stats(s.multi, &st) != ADYPT_OK) return tracer_failed(s.multi);
	printf("[PT]INFO: %d spp on %d GPU%s, %llu rays in %.1f ms wall (%.1f Mrays/s; traversal kernels %.1f ms, shade kernels %.1f ms)\n",
		   adypt_multi_get_spp(s.multi), (int)o.devices.size(), o.devices.size() > 1 ? "s" : "", (unsigned long long)st.rays, s.render_ms,
		   st.rays / (s.render_ms * 1e3), st.trace_ms, st.shade_ms);
	if(!save(s)) return false;
	printf("[PT]INFO: Saved image to %s\n", o.out.c_str());
	if(!o.preview.empty()) printf("[PT]INFO: Saved preview to %s\n", o.preview.c_str());
	return true;
}

// one float per pixel as a grey EXR
static bool save_grey(const Session &s, const std::string &path, const std::vector<float> &values, const char *label)
{
	std::vector<float> grey(values.size() * 3);
	for(size_t i = 0; i < values.size(); ++i) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = values[i];
	if(adypt_save_exr(path.c_str(), grey.data(), s.cfg.width, s.cfg.height, 0) != ADYPT_OK) return host_failed();
	printf("[PT]INFO: Saved %s to %s\n", label, path.c_str());
	return true;
}

// the sample count of every pixel from the devices' blocks (every block has one owner)
static bool pixel_spp(const Session &s, std::vector<float> *count_of)
{
	const int w = s.cfg.width, h = s.cfg.height;
	count_of->assign((size_t)w * h, 0.0f);
	const int blocks_x = (w + 31) / 32;
	for(size_t k = 0; k < s.opt.devices.size(); ++k)
	{
		adypt_ctx *c = adypt_multi_context(s.multi, (int)k);
		const int64_t n = adypt_read_block_spp(c, nullptr, nullptr, 0);
		std::vector<int32_t> index((size_t)std::max<int64_t>(n, 0)), count(index.size());
		if(n < 0 || (n > 0 && adypt_read_block_spp(c, index.data(), count.data(), n) != n)) { fprintf(stderr, "[TRACER]Err: %s\n", adypt_last_error(c)); return false; }
		for(size_t b = 0; b < index.size(); ++b)
			for(int y = (index[b] / blocks_x) * 32; y < std::min(h, (index[b] / blocks_x + 1) * 32); ++y)
				for(int x = (index[b] % blocks_x) * 32; x < std::min(w, (index[b] % blocks_x + 1) * 32); ++x) (*count_of)[(size_t)y * w + x] = (float)count[b];
	}
	return true;
}

// --history-samples: its line and its images
static bool report_plan(Session &s)
{
	const Options &o = s.opt;
	if(!o.history_samples) return true;
	const adypt_history_plan &plan = s.plan;
	printf("[PT]PLAN: blocks %d want %d..%d pixel_samples %lld (uniform %lld) with_history %lld of %lld mean_reach %.3f\n", plan.blocks, plan.want_min, plan.want_max, (long long)plan.pixel_samples,
	       (long long)*o.history_samples * plan.pixels, (long long)plan.pixels_with_history, (long long)plan.pixels, plan.mean_reach);
	if(!o.reach_out.empty())
	{
		std::vector<float> reach((size_t)s.cfg.width * s.cfg.height, 0.0f);
		if(adypt_multi_read_history_reach(s.multi, reach.data()) != ADYPT_OK) return tracer_failed(s.multi);
		if(!save_grey(s, o.reach_out, reach, "history reach")) return false;
	}
	if(!o.plan_out.empty())
	{
		const int w = s.cfg.width, h = s.cfg.height, blocks_x = (w + 31) / 32;
		std::vector<int32_t> index((size_t)plan.blocks), want(index.size());
		if(adypt_multi_read_sample_plan(s.multi, index.data(), want.data(), plan.blocks) != plan.blocks) return tracer_failed(s.multi);
		std::vector<float> want_of((size_t)w * h, 0.0f);
		for(size_t b = 0; b < index.size(); ++b)
			for(int y = (index[b] / blocks_x) * 32; y < std::min(h, (index[b] / blocks_x + 1) * 32); ++y)
				for(int x = (index[b] % blocks_x) * 32; x < std::min(w, (index[b] % blocks_x + 1) * 32); ++x) want_of[(size_t)y * w + x] = (float)want[b];
		if(!save_grey(s, o.plan_out, want_of, "planned sample counts")) return false;
	}
	return true;
}

// --noise: its images and its line
static bool report_noise(Session &s)
{
	const Options &o = s.opt;
	const adypt_noise &noise = s.noise;
	if(!o.until) return true;
	if(!o.noise_out.empty())
	{
		std::vector<float> e((size_t)s.cfg.width * s.cfg.height, 0.0f);
		if(adypt_multi_read_noise(s.multi, e.data()) != ADYPT_OK) return tracer_failed(s.multi);
		if(!save_grey(s, o.noise_out, e, "noise")) return false;
	}
	if(!o.spp_out.empty())
	{
		std::vector<float> count_of;
		if(!pixel_spp(s, &count_of) || !save_grey(s, o.spp_out, count_of, "sample counts")) return false;
	}
	if(o.adaptive)
		printf("[PT]ADAPTIVE: spp %d frozen %d of %d pixel_samples %lld (uniform %lld) mean_noise %.9g worst_block %.9g worst_index %d (target %.9g)\n", noise.spp, s.adapt.blocks_frozen,
		       s.adapt.blocks, (long long)s.adapt.pixel_samples, (long long)noise.spp * (long long)s.cfg.width * (long long)s.cfg.height, noise.mean_noise, noise.worst_block, noise.worst_index, o.noise_target);
	else printf("[PT]NOISE: spp %d mean_noise %.9g worst_block %.9g worst_index %d (target %.9g)\n", noise.spp, noise.mean_noise, noise.worst_block, noise.worst_index, o.noise_target);
	return true;
}

// the [PT]TEMPORAL: line and the images of the last temporal call.  On the host from the read-backs: a hit pixel found history when its effective
// sample count is above its block's own
static bool report_temporal(Session &s)
{
	const Options &o = s.opt;
	std::vector<float> length((size_t)s.cfg.width * s.cfg.height, 0.0f), count_of, kept;
	std::vector<uint8_t> hit(length.size(), 0);
	if(adypt_multi_read_denoise_history(s.multi, length.data()) != ADYPT_OK || adypt_multi_read_denoise_guides(s.multi, nullptr, nullptr, nullptr, hit.data()) != ADYPT_OK) return tracer_failed(s.multi);
	if(!pixel_spp(s, &count_of)) return false;
	long long hits = 0, with_history = 0;
	double sum = 0.0;
	for(size_t i = 0; i < length.size(); ++i)
		if(hit[i]) { ++hits; sum += length[i]; if(length[i] > count_of[i]) ++with_history; }
	printf("[PT]TEMPORAL: history on %lld of %lld hit pixels, mean length %.3f", with_history, hits, hits ? sum / (double)hits : 0.0);
	if(o.follow_motion)
	{
		std::vector<uint8_t> moved(length.size(), 0);
		if(adypt_multi_read_denoise_motion(s.multi, nullptr, moved.data()) != ADYPT_OK) return tracer_failed(s.multi, "\n");
		printf(", moved %lld pixels", (long long)std::count(moved.begin(), moved.end(), (uint8_t)1));
	}
	if(o.rectify)
	{
		kept.assign(length.size(), 1.0f);
		if(adypt_multi_read_denoise_rectify(s.multi, kept.data()) != ADYPT_OK) return tracer_failed(s.multi, "\n");
		printf(", rectified %lld pixels", (long long)std::count_if(kept.begin(), kept.end(), [](float k) { return k < 1.0f; }));
	}
	std::vector<float> variance;
	if(o.denoise_moments)
	{
		adypt_denoise_moments info;
		variance.assign(length.size(), 0.0f);
		if(adypt_multi_get_denoise_moments(s.multi, &info) != ADYPT_OK || adypt_multi_read_denoise_variance(s.multi, variance.data()) != ADYPT_OK) return tracer_failed(s.multi, "\n");
		printf(", spatial variance on %lld pixels", (long long)info.pixels_spatial);
	}
	if(o.follow_specular)
	{
		adypt_denoise_virtual info;
		if(adypt_multi_get_denoise_virtual(s.multi, &info) != ADYPT_OK) return tracer_failed(s.multi, "\n");
		printf(", followed %lld pixels, %lld with history", (long long)info.pixels_followed, (long long)info.pixels_with_history);
	}
	printf("\n");
	if(!o.rectify_out.empty() && !save_grey(s, o.rectify_out, kept, "kept history shares")) return false;
	if(!o.variance_out.empty() && !save_grey(s, o.variance_out, variance, "variance")) return false;
	return o.history_out.empty() || save_grey(s, o.history_out, length, "history lengths");
}

// the [PT]SPECULAR: line of the last call with followed guides: the chain's own counts, and the hit pixels from its class codes
static bool report_specular(Session &s)
{
	adypt_denoise_specular_info info;
	std::vector<int8_t> chain((size_t)s.cfg.width * s.cfg.height, 0);
	if(adypt_multi_read_denoise_guides_specular(s.multi, *s.opt.denoise_specular, nullptr, nullptr, nullptr, chain.data()) != ADYPT_OK || adypt_multi_get_denoise_specular(s.multi, &info) != ADYPT_OK)
		return tracer_failed(s.multi);
	const long long hits = (long long)std::count_if(chain.begin(), chain.end(), [](int8_t c) { return c != 0; });
	printf("[PT]SPECULAR: bounces %d followed %lld escaped %lld truncated %lld of %lld hit pixels, rays %lld\n", info.bounces, (long long)info.pixels_followed, (long long)info.pixels_escaped,
	       (long long)info.pixels_truncated, hits, (long long)info.rays);
	return true;
}

static bool save_denoised(Session &s)
{
	const Options &o = s.opt;
	if(!o.denoise) return true;
	std::vector<float> den((size_t)s.cfg.width * s.cfg.height * 3, 0.0f);
	const adypt_specular_params specular{o.denoise_specular.value_or(0)};
	const int r = o.temporal ? temporal_call(s) : o.denoise_specular ? adypt_multi_denoise_specular(s.multi, &s.denoise_params, &specular) : adypt_multi_denoise(s.multi, &s.denoise_params);
	if(r != ADYPT_OK || adypt_multi_read_denoised(s.multi, den.data()) != ADYPT_OK) return tracer_failed(s.multi);
	if(adypt_save_exr(o.denoise_out.c_str(), den.data(), s.cfg.width, s.cfg.height, o.fp16) != ADYPT_OK) return host_failed();
	printf("[PT]INFO: Saved denoised image (%d levels) to %s\n", o.denoise_levels, o.denoise_out.c_str());
	if(o.denoise_specular && !report_specular(s)) return false;
	return !o.temporal || report_temporal(s);
}

static bool save_guides(Session &s)
{
	const std::string &prefix = s.opt.guides_out;
	if(prefix.empty()) return true;
	std::vector<float> g[3];
	for(auto &v : g) v.assign((size_t)s.cfg.width * s.cfg.height * 3, 0.0f);
	const std::optional<int> &bounces = s.opt.denoise_specular ? s.opt.denoise_specular : s.opt.follow_specular; // (the followed guides, and the class codes beside them)
	std::vector<int8_t> chain(bounces ? (size_t)s.cfg.width * s.cfg.height : 0, 0);
	const int r = bounces ? adypt_multi_read_denoise_guides_specular(s.multi, *bounces, g[0].data(), g[1].data(), g[2].data(), chain.data())
	                      : adypt_multi_read_denoise_guides(s.multi, g[0].data(), g[1].data(), g[2].data(), nullptr);
	if(r != ADYPT_OK) return tracer_failed(s.multi);
	const char *const what[3] = {".albedo.exr", ".normal.exr", ".position.exr"};
	for(int k = 0; k < 3; ++k)
		if(adypt_save_exr((prefix + what[k]).c_str(), g[k].data(), s.cfg.width, s.cfg.height, 0) != ADYPT_OK) return host_failed();
	printf("[PT]INFO: Saved guide images to %s.{albedo,normal,position}.exr\n", prefix.c_str());
	return !bounces || save_grey(s, prefix + ".chain.exr", std::vector<float>(chain.begin(), chain.end()), "chain classes");
}

// like ~Instance (src/Instance.cpp:83-86): the config is written back on exit — the successful one
static void release(Session &s)
{
	adypt_destroy_multi(s.multi);
	if(s.bvh) adypt_bvh_free(s.bvh);
	adypt_scene_free(s.scene);
	if(s.appearance) adypt_scene_free(s.appearance);
	adypt_config_save(s.opt.config.c_str(), &s.cfg);
}

int main(int argc, char **argv)
{
	Session s;
	int code = parse_options(argc, argv, &s.opt);
	if(code != GO_ON) return code;
	if(s.opt.test_hooks) (void)adypt_enable_test_hooks(ADYPT_TEST_HOOKS_MAGIC);
	if((code = check_options(&s.opt)) != GO_ON) return code;
	const bool follow = s.opt.follow_motion; // the history poses then show the scene as loaded, with its snapshot; a pose leaves the tracer at 0 spp
	if(!load_inputs(s) || !create_tracer(s)) return 1;
	if(!follow && !move_scene(s)) return 1;
	if(!commit_history_poses(s)) return 1;
	if(follow && !move_scene(s)) return 1;
	if(!swap_materials(s) || !back_to_the_main_view(s) || !render(s)) return 1;
	if(!report_and_save_image(s) || !report_noise(s) || !report_plan(s) || !save_denoised(s) || !save_guides(s)) return 1;
	release(s);
	return 0;
}
