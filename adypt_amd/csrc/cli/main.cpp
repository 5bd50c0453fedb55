// adypt_hip — headless equivalent of the reference application for one .config file:
//   Instance::InitializeFromFile / Initialize (src/Instance.cpp:10-42,59-69) -> N x Trace(true) -> SaveResult
//   (src/Tracer/OglPathTracer.cpp:199-212).  The interactive window / ImGui front-end is out of scope.
//
//   adypt_hip scene.config [--spp N] [--out result.exr] [--fp16] [--primary TYPE] [--preview file.png] [--sun-visibility] [--seed S]
//             [--device D | --devices D0,D1,...] [--save-every K] [--noise T [--min-spp N] [--check-every K] [--noise-out file.exr]
//             [--adaptive [--spp-out file.exr]]] [--denoise file.exr [--denoise-levels L] [--history-from other.config]... [--history-cap C]
//             [--history-out len.exr] [--follow-motion] [--rectify [--rectify-gamma G] [--rectify-radius R] [--rectify-out kept.exr]]] [--guides-out PREFIX] [--pose moved.obj | --part-matrices FILE] [--morph-target FILE.obj]... [--morph-weights w0,w1,...] [--rebuild] [--rebuild-method linear|ploc [--ploc-radius R] [--split-budget B]] [--rebuild-above R] [--build gpu]
//   --build gpu: no .bvh cache is read or written and no tree is built on the host: the context is created from the triangles alone
//              (adypt_create_multi_from_triangles) and its first tree built on the GPU by --rebuild-method (ploc unless given), --ploc-radius and
//              --split-budget, which then name that build (and, with --rebuild-above, the policy's rebuild) instead of asking for a rebuild; one
//              [PT]BUILD: line reports it.  --pose and --rebuild-above work after it as they do otherwise; a bare --rebuild with it, or any other word than gpu (or host, the default), is exit 2
//   --pose moved.obj: the scene of the config (and its cached .bvh) with the vertices and normals of moved.obj — the same triangles in the same order,
//              moved — through adypt_multi_update_triangles: the BVH and the Woop data are refitted on the GPU, nothing is rebuilt
//   --part-matrices FILE: the scene moved on the GPU, part by part (adypt_multi_bind_parts, adypt_multi_pose): a triangle's part is its material id, and
//              triangles without a material (id -1) are one extra last part.  FILE holds lines `part m00 m01 m02 m03 m10 ... m23` (a row-major 3x4
//              matrix: three linear entries and the translation per row; # starts a comment); parts that are not listed stay where they are.  One
//              [PT]POSE: line reports it.  --rebuild-above and the options that name its rebuild work as after --pose; together with --pose: exit 2
//   --morph-target FILE.obj (repeatable) with --morph-weights w0,w1,...: blend shapes on the GPU.  Target k is the k-th FILE given — the scene's
//              triangles in the same order, moved — and is diffed against the scene as loaded (adypt_morph_diff); the entries are bound as one layer on
//              the parts binding of --part-matrices (parts by material id; without --part-matrices every matrix is the identity) and posed once with
//              the weights (adypt_multi_bind_morph, adypt_multi_pose_morph).  One [PT]MORPH: line reports targets, entries and triangles touched.
//              --rebuild-above works as after --part-matrices.  One option without the other, a weight count other than the target count, or either
//              together with --pose: exit 2
//   --rebuild: a new tree for the triangles as they are then (after --pose, when given), built on the GPU through adypt_multi_rebuild_bvh with the config's
//              SAH costs
//   --rebuild-method ploc: the same with the binary tree built by PLOC (adypt_multi_rebuild_bvh_ploc; --ploc-radius R, 1 to 32, 8 unless given) — a tighter
//              tree for a few times the build time; linear (the default) is --rebuild's tree.  Naming a method asks for the rebuild
//   --split-budget B: with --rebuild-method ploc only (else exit 2): large triangles are split into several references first, at most B * n more than
//              triangles, B in [0, 1] (adypt_multi_rebuild_bvh_ploc_split)
//   --rebuild-above R: with --pose or --part-matrices only, and not with a bare --rebuild (else exit 2): the pose goes through adypt_multi_update_triangles_auto — the tree is
//              refitted, its SAH cost measured, and rebuilt only where that is more than R times the cost of the tree as loaded (R finite and >= 0, no
//              default; 0 always rebuilds).  --rebuild-method, --ploc-radius and --split-budget then name the rebuild of that policy (linear unless
//              given) instead of asking for one outright
//   --sun-visibility: enable the occlusion query the reference has commented out (pathtracer.glsl:132)
//   --preview: what the reference shows in its window (shaders/screen.glsl), as PNG
//   --devices: pixel tiles sharded over several GPUs of the node (adypt_create_multi), radiance gathered on the first one
//   --save-every K: progressive rendering as in the reference's window — the running mean is written to --out (and --preview)
//                   every K samples; the file on disk is always a complete image of what has converged so far
//   --noise T: render until the noisiest 32x32 block of the image is at or below T (adypt_multi_trace_until: the relative standard error of the mean
//              luminance, adypt_hip.h); --spp is then the cap, --min-spp (default 16) the least, and the noise is looked at every --check-every
//              (default 16) samples.  --noise-out: the per-pixel noise as a grey EXR
//   --adaptive: with --noise T, every 32x32 block stops being traced at the check at which ITS mean noise is at or below T (adypt_multi_trace_adaptive);
//              the render ends when every block has stopped, or at --spp.  --spp-out: the per-pixel sample count as a grey EXR
//   --denoise file.exr: the image through the variance- and primary-hit-guided a-trous filter (adypt_multi_denoise) next to --out; switches the noise
//              statistics on before the first sample, as --noise does; needs --spp >= 2 and no --primary.  --denoise-levels L: 1 .. 6 levels (default 5)
//   --history-from other.config: with --denoise only; repeatable, run in order before the render.  The other config names the same OBJ, width and
//              height (else exit 1); for each one: that config's camera, --spp samples with shift_seed = --seed + 1 + its index, and a committing temporal
//              call (adypt_multi_denoise_temporal).  Then the main config's camera and --seed, a reset of the accumulation, the render as without it, and a
//              temporal call into the --denoise file.  --history-cap C: the most samples the history counts as (a positive finite number, default 64).
//              --history-out len.exr: the effective sample count of every pixel after that call as a grey EXR.  One [PT]TEMPORAL: line reports how many
//              hit pixels found history.  --history-cap or --history-out without --history-from make the --denoise call a temporal one too: it finds no
//              history, so the file holds the plain filter's bits, every length is the block's own sample count and the line reports 0 pixels
//   --follow-motion: with a temporal --denoise call only (one of the --history options; else exit 2): every temporal call is a motion call
//              (adypt_multi_denoise_temporal_motion), and the --history-from poses are rendered and committed BEFORE --pose / --part-matrices (and the rebuild
//              that goes with them) is applied — they show the scene as loaded, the main render the moved one, and pixels on moved triangles find
//              their history through the pose they had.  The [PT]TEMPORAL: line then ends `, moved M pixels`.  Without it the pose comes first
//   --rectify: with a temporal --denoise call only (else exit 2): every temporal call is a rectified one (adypt_multi_denoise_temporal_rectified) — the
//              history is held against the mean of the window of the call's own image on the pixel's surface, clamped to within --rectify-gamma G
//              standard deviations of it (a finite number >= 0, default 1; window radius --rectify-radius R, 1 .. 3, default 3) and loses length by as
//              much as it disagrees: for light that changed on a surface that stands still.  Combines with --follow-motion.  --rectify-out kept.exr: the
//              share of its length every pixel's history kept, as a grey EXR.  The [PT]TEMPORAL: line then ends `, rectified K pixels`: those with a
//              share below 1.  --rectify-gamma, --rectify-radius and --rectify-out need --rectify
//   --guides-out PREFIX: the feature images of the primary hit as PREFIX.albedo.exr, PREFIX.normal.exr and PREFIX.position.exr
#include "adypt_hip.h"
#include "adypt_host.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char **argv)
{
	if(argc < 2) { fprintf(stderr, "usage: %s scene.config [--spp N] [--out file.exr] [--fp16] [--primary TYPE] [--preview file.png] [--sun-visibility] [--seed S] [--device D | --devices D0,D1,...] [--save-every K] [--noise T [--min-spp N] [--check-every K] [--noise-out file.exr] [--adaptive [--spp-out file.exr]]] [--denoise file.exr [--denoise-levels L] [--history-from other.config]... [--history-cap C] [--history-out len.exr] [--follow-motion] [--rectify [--rectify-gamma G] [--rectify-radius R] [--rectify-out kept.exr]]] [--guides-out PREFIX] [--pose moved.obj | --part-matrices FILE] [--rebuild] [--rebuild-method linear|ploc [--ploc-radius R] [--split-budget B]] [--rebuild-above R] [--build gpu]\n", argv[0]); return 2; }
	int min_spp = 16, check_every = 16;
	double noise_target = -1.0; // < 0: render to a fixed sample count
	std::string noise_out, spp_out, denoise_out, guides_out, pose, part_matrices;
	std::vector<std::string> morph_targets;
	std::vector<float> morph_weights;
	bool have_morph_weights = false;
	bool rebuild = false, bare_rebuild = false, have_rebuild_above = false;
	double rebuild_above = 0.0;
	std::string rebuild_method = "linear";
	double split_budget = 0.0;
	bool have_split_budget = false, have_rebuild_method = false, build_on_gpu = false;
	int ploc_radius = 8;
	int denoise_levels = 5;
	std::vector<std::string> history_from;
	std::string history_out;
	double history_cap = 64.0;
	bool have_history_cap = false, follow_motion = false;
	bool rectify = false, have_rectify_option = false;
	adypt_rectify_params rp{3, 1.0f};
	std::string rectify_out;
	int adaptive = 0;
	int spp = 64, fp16 = 0, primary = -1, sun_visibility = 0, save_every = 0;
	std::vector<int> devices(1, 0);
	unsigned seed = 12345;
	std::string out = "result.exr", preview;
	for(int i = 2; i < argc; ++i)
	{
		std::string a = argv[i];
		if(a == "--spp" && i + 1 < argc) spp = atoi(argv[++i]);
		else if(a == "--out" && i + 1 < argc) out = argv[++i];
		else if(a == "--preview" && i + 1 < argc) preview = argv[++i];
		else if(a == "--fp16") fp16 = 1;
		else if(a == "--sun-visibility") sun_visibility = 1;
		else if(a == "--test-hooks") (void)adypt_enable_test_hooks(ADYPT_TEST_HOOKS_MAGIC); // tests only: lets ADYPT_MULTI_SHARED_DEVICE put several shards on one device
		else if(a == "--primary" && i + 1 < argc) primary = atoi(argv[++i]);
		else if(a == "--seed" && i + 1 < argc) seed = (unsigned)strtoul(argv[++i], nullptr, 10);
		else if(a == "--device" && i + 1 < argc) devices.assign(1, atoi(argv[++i]));
		else if(a == "--devices" && i + 1 < argc)
		{
			devices.clear();
			for(const char *q = argv[++i]; *q;)
			{
				char *end = nullptr;
				const long v = strtol(q, &end, 10);
				if(end == q || v < 0) { fprintf(stderr, "bad --devices list %s\n", argv[i]); return 2; }
				devices.push_back((int)v);
				q = *end == ',' ? end + 1 : end;
				if(*end && *end != ',') { fprintf(stderr, "bad --devices list %s\n", argv[i]); return 2; }
			}
			if(devices.empty()) { fprintf(stderr, "empty --devices list\n"); return 2; }
		}
		else if(a == "--save-every" && i + 1 < argc) save_every = atoi(argv[++i]);
		else if(a == "--noise" && i + 1 < argc) noise_target = atof(argv[++i]);
		else if(a == "--min-spp" && i + 1 < argc) min_spp = atoi(argv[++i]);
		else if(a == "--check-every" && i + 1 < argc) check_every = atoi(argv[++i]);
		else if(a == "--noise-out" && i + 1 < argc) noise_out = argv[++i];
		else if(a == "--adaptive") adaptive = 1;
		else if(a == "--spp-out" && i + 1 < argc) spp_out = argv[++i];
		else if(a == "--denoise" && i + 1 < argc) denoise_out = argv[++i];
		else if(a == "--denoise-levels" && i + 1 < argc) denoise_levels = atoi(argv[++i]);
		else if(a == "--history-from" && i + 1 < argc) history_from.push_back(argv[++i]);
		else if(a == "--history-out" && i + 1 < argc) history_out = argv[++i];
		else if(a == "--history-cap" && i + 1 < argc)
		{
			char *end = nullptr;
			history_cap = strtod(argv[++i], &end);
			if(end == argv[i] || *end || !(history_cap > 0.0 && history_cap <= 3.0e38)) { fprintf(stderr, "--history-cap takes a positive finite number, not %s\n", argv[i]); return 2; }
			have_history_cap = true;
		}
		else if(a == "--follow-motion") follow_motion = true;
		else if(a == "--rectify") rectify = true;
		else if(a == "--rectify-out" && i + 1 < argc) { rectify_out = argv[++i]; have_rectify_option = true; }
		else if(a == "--rectify-radius" && i + 1 < argc)
		{
			char *end = nullptr;
			const long v = strtol(argv[++i], &end, 10);
			if(end == argv[i] || *end || v < 1 || v > 3) { fprintf(stderr, "--rectify-radius takes 1, 2 or 3, not %s\n", argv[i]); return 2; }
			rp.radius = (int32_t)v; have_rectify_option = true;
		}
		else if(a == "--rectify-gamma" && i + 1 < argc)
		{
			char *end = nullptr;
			const double v = strtod(argv[++i], &end);
			if(end == argv[i] || *end || !(v >= 0.0 && v <= 3.0e38)) { fprintf(stderr, "--rectify-gamma takes a finite number that is not negative, not %s\n", argv[i]); return 2; }
			rp.gamma = (float)v; have_rectify_option = true;
		}
		else if(a == "--guides-out" && i + 1 < argc) guides_out = argv[++i];
		else if(a == "--pose" && i + 1 < argc) pose = argv[++i];
		else if(a == "--part-matrices" && i + 1 < argc) part_matrices = argv[++i];
		else if(a == "--morph-target" && i + 1 < argc) morph_targets.push_back(argv[++i]);
		else if(a == "--morph-weights" && i + 1 < argc)
		{
			have_morph_weights = true;
			morph_weights.clear();
			for(const char *q = argv[++i];;)
			{
				char *end;
				const float v = strtof(q, &end);
				if(end == q || (*end && *end != ',')) { fprintf(stderr, "bad --morph-weights list %s\n", argv[i]); return 2; }
				morph_weights.push_back(v);
				if(!*end) break;
				q = end + 1;
			}
		}
		else if(a == "--rebuild") rebuild = bare_rebuild = true;
		else if(a == "--rebuild-above" && i + 1 < argc)
		{
			char *end = nullptr;
			rebuild_above = strtod(argv[++i], &end);
			if(end == argv[i] || *end || !(rebuild_above >= 0.0 && rebuild_above < HUGE_VAL)) { fprintf(stderr, "--rebuild-above takes a finite number >= 0, not %s\n", argv[i]); return 2; }
			have_rebuild_above = true;
		}
		else if(a == "--rebuild-method" && i + 1 < argc) { rebuild_method = argv[++i]; rebuild = have_rebuild_method = true; }
		else if(a == "--build" && i + 1 < argc)
		{
			const std::string where = argv[++i];
			if(where != "gpu" && where != "host") { fprintf(stderr, "--build is gpu or host, not %s\n", where.c_str()); return 2; }
			build_on_gpu = where == "gpu";
		}
		else if(a == "--ploc-radius" && i + 1 < argc) ploc_radius = atoi(argv[++i]);
		else if(a == "--split-budget" && i + 1 < argc) { split_budget = atof(argv[++i]); have_split_budget = true; }
		else { fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
	}
	const bool until = noise_target >= 0.0;
	if(build_on_gpu && bare_rebuild) { fprintf(stderr, "--build gpu has just built the tree: name its method with --rebuild-method, without --rebuild\n"); return 2; }
	if(build_on_gpu && !have_rebuild_method) rebuild_method = "ploc";
	if(rebuild_method != "linear" && rebuild_method != "ploc") { fprintf(stderr, "--rebuild-method is linear or ploc\n"); return 2; }
	if(have_split_budget && rebuild_method != "ploc") { fprintf(stderr, "--split-budget needs --rebuild-method ploc\n"); return 2; }
	if(!pose.empty() && !part_matrices.empty()) { fprintf(stderr, "--pose and --part-matrices are two ways to move the scene: give one\n"); return 2; }
	const bool morphing = !morph_targets.empty();
	if(morphing != have_morph_weights) { fprintf(stderr, "--morph-target FILE.obj and --morph-weights w0,w1,... go together\n"); return 2; }
	if(morphing && morph_weights.size() != morph_targets.size()) { fprintf(stderr, "--morph-weights has %d weights for %d --morph-target\n", (int)morph_weights.size(), (int)morph_targets.size()); return 2; }
	if(morphing && !pose.empty()) { fprintf(stderr, "--morph-target morphs the scene as loaded: not together with --pose\n"); return 2; }
	if(have_rebuild_above && pose.empty() && part_matrices.empty() && !morphing) { fprintf(stderr, "--rebuild-above needs --pose moved.obj, --part-matrices FILE or --morph-target\n"); return 2; }
	if(have_rebuild_above && bare_rebuild) { fprintf(stderr, "--rebuild-above decides about the rebuild itself: name its method with --rebuild-method, without --rebuild\n"); return 2; }
	if(have_rebuild_above || build_on_gpu) rebuild = false; // (--rebuild-method names the policy's rebuild, or the first build)
	// the tree that --rebuild-method, --ploc-radius and --split-budget name: the first build of --build gpu, the policy's rebuild, or the rebuild asked for
	const bool ploc = rebuild_method == "ploc";
	const adypt_pose_policy policy{rebuild_above, ploc ? 1 : 0, ploc_radius, split_budget};
	if(!until && !noise_out.empty()) { fprintf(stderr, "--noise-out needs --noise T\n"); return 2; }
	if(until && (primary >= 0 || spp < 2 || check_every < 1)) { fprintf(stderr, "--noise needs --spp >= 2, --check-every >= 1 and no --primary\n"); return 2; }
	if(adaptive && (!until || save_every > 0)) { fprintf(stderr, "--adaptive needs --noise T and does not combine with --save-every\n"); return 2; }
	if(!adaptive && !spp_out.empty()) { fprintf(stderr, "--spp-out needs --adaptive\n"); return 2; }
	const bool denoise = !denoise_out.empty();
	if(denoise && (primary >= 0 || spp < 2)) { fprintf(stderr, "--denoise needs --spp >= 2 and no --primary\n"); return 2; }
	if(denoise && (denoise_levels < 1 || denoise_levels > 6)) { fprintf(stderr, "--denoise-levels must be in 1 .. 6\n"); return 2; }
	const bool temporal = !history_from.empty() || have_history_cap || !history_out.empty();
	if(temporal && !denoise) { fprintf(stderr, "--history-from, --history-cap and --history-out need --denoise file.exr\n"); return 2; }
	if(have_rectify_option && !rectify) { fprintf(stderr, "--rectify-gamma, --rectify-radius and --rectify-out need --rectify\n"); return 2; }
	if(rectify && !temporal) { fprintf(stderr, "--rectify needs a temporal --denoise call: --denoise file.exr with --history-from, --history-cap or --history-out\n"); return 2; }
	if(follow_motion && !temporal) { fprintf(stderr, "--follow-motion needs a temporal --denoise call: --denoise file.exr with --history-from, --history-cap or --history-out\n"); return 2; }
	if(until) min_spp = std::max(2, std::min(min_spp, spp));
	adypt_config cfg;
	adypt_config_default(&cfg);
	if(adypt_config_load(argv[1], &cfg) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Invalid instance %s: %s\n", argv[1], adypt_host_last_error()); return 1; }
	printf("[INSTANCE]Info: Instance loaded from %s\n", argv[1]);
	std::vector<adypt_config> history_cfg(history_from.size()); // --history-from: the earlier poses, of which only the cameras are used
	for(size_t k = 0; k < history_from.size(); ++k)
	{
		adypt_config_default(&history_cfg[k]);
		if(adypt_config_load(history_from[k].c_str(), &history_cfg[k]) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Invalid instance %s: %s\n", history_from[k].c_str(), adypt_host_last_error()); return 1; }
		if(strcmp(history_cfg[k].obj_filename, cfg.obj_filename) != 0 || history_cfg[k].width != cfg.width || history_cfg[k].height != cfg.height)
		{
			fprintf(stderr, "[INSTANCE]Err: --history-from %s names another scene or another size than %s (%s, %d x %d)\n", history_from[k].c_str(), argv[1], cfg.obj_filename, cfg.width, cfg.height);
			return 1;
		}
	}

	adypt_scene *scene = nullptr;
	if(adypt_scene_load(cfg.obj_filename, &scene) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Unable to load scene %s: %s\n", cfg.obj_filename, adypt_host_last_error()); return 1; }
	const void *tris, *mats, *tex;
	int64_t n_tris = adypt_scene_triangles(scene, &tris), n_mats = adypt_scene_materials(scene, &mats);
	int32_t n_tex = adypt_scene_textures(scene, &tex);
	printf("[SCENE]Info: %lld triangles loaded from %s\n", (long long)n_tris, cfg.obj_filename);
	if(*adypt_scene_warnings(scene)) printf("[SCENE]Warn: %s", adypt_scene_warnings(scene)); // undecodable textures: their materials render black

	std::vector<float> pose_positions, pose_normals; // --pose: what replaces the scene's vertices and normals once the context exists
	if(!pose.empty())
	{
		adypt_scene *moved = nullptr;
		if(adypt_scene_load(pose.c_str(), &moved) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Unable to load pose %s: %s\n", pose.c_str(), adypt_host_last_error()); return 1; }
		const void *mt;
		const int64_t n_moved = adypt_scene_triangles(moved, &mt);
		if(n_moved != n_tris) { fprintf(stderr, "[INSTANCE]Err: pose %s has %lld triangles, the scene has %lld\n", pose.c_str(), (long long)n_moved, (long long)n_tris); return 1; }
		pose_positions.resize((size_t)n_tris * 9); pose_normals.resize((size_t)n_tris * 9);
		for(int64_t i = 0; i < n_tris; ++i) // (100-byte records: 9 position floats, 9 normal floats, ...)
		{
			memcpy(&pose_positions[(size_t)i * 9], (const uint8_t *)mt + i * 100, 36);
			memcpy(&pose_normals[(size_t)i * 9], (const uint8_t *)mt + i * 100 + 36, 36);
		}
		adypt_scene_free(moved);
	}

	std::vector<int32_t> part_of_triangle; // --part-matrices: the binding and one matrix per part, the identity where FILE names none
	std::vector<float> part_matrix;
	int32_t n_parts = 0;
	if(!part_matrices.empty() || morphing)
	{
		part_of_triangle.resize((size_t)n_tris);
		bool loose = false;
		for(int64_t i = 0; i < n_tris; ++i) // (100-byte records: the material id is the last word)
		{
			int32_t matid;
			memcpy(&matid, (const uint8_t *)tris + i * 100 + 96, 4);
			const bool known = matid >= 0 && matid < n_mats;
			part_of_triangle[(size_t)i] = known ? matid : (int32_t)n_mats;
			loose |= !known;
		}
		n_parts = (int32_t)n_mats + (loose ? 1 : 0);
		for(int32_t k = 0; k < n_parts; ++k)
			for(int j = 0; j < 12; ++j) part_matrix.push_back(j % 5 == 0 ? 1.0f : 0.0f);
		FILE *f = part_matrices.empty() ? nullptr : fopen(part_matrices.c_str(), "r");
		if(!f && !part_matrices.empty()) { fprintf(stderr, "[INSTANCE]Err: Unable to open %s\n", part_matrices.c_str()); return 1; }
		char line[1024];
		for(int at = 1; f && fgets(line, sizeof(line), f); ++at)
		{
			if(char *hash = strchr(line, '#')) *hash = 0;
			long part;
			float m[12];
			int used = 0;
			const int got = sscanf(line, "%ld %f %f %f %f %f %f %f %f %f %f %f %f %n", &part, m, m + 1, m + 2, m + 3, m + 4, m + 5, m + 6, m + 7, m + 8, m + 9, m + 10, m + 11, &used);
			if(got <= 0 && line[strspn(line, " \t\r\n")] == 0) continue;
			if(got != 13 || line[used] != 0 || part < 0 || part >= n_parts)
			{
				fprintf(stderr, "[INSTANCE]Err: %s line %d is not `part m00 ... m23` with a part in [0, %d)\n", part_matrices.c_str(), at, (int)n_parts);
				fclose(f);
				return 1;
			}
			memcpy(&part_matrix[(size_t)part * 12], m, sizeof(m));
		}
		if(f) fclose(f);
	}

	std::vector<int32_t> morph_triangle, morph_target; // --morph-target: the entries of all targets, each diffed against the scene as loaded
	std::vector<float> morph_deltas;
	for(size_t k = 0; k < morph_targets.size(); ++k)
	{
		adypt_scene *target = nullptr;
		if(adypt_scene_load(morph_targets[k].c_str(), &target) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Unable to load morph target %s: %s\n", morph_targets[k].c_str(), adypt_host_last_error()); return 1; }
		const void *tt;
		const int64_t n_target = adypt_scene_triangles(target, &tt);
		if(n_target != n_tris) { fprintf(stderr, "[INSTANCE]Err: morph target %s has %lld triangles, the scene has %lld\n", morph_targets[k].c_str(), (long long)n_target, (long long)n_tris); return 1; }
		const int64_t count = adypt_morph_diff(tris, tt, n_tris, nullptr, nullptr);
		if(count < 0) { fprintf(stderr, "[INSTANCE]Err: %s\n", adypt_host_last_error()); return 1; }
		const size_t at = morph_triangle.size();
		morph_triangle.resize(at + (size_t)count);
		morph_deltas.resize((at + (size_t)count) * 18);
		morph_target.resize(at + (size_t)count, (int32_t)k);
		(void)adypt_morph_diff(tris, tt, n_tris, morph_triangle.data() + at, morph_deltas.data() + at * 18);
		adypt_scene_free(target);
	}

	adypt_bvh *bvh = nullptr;
	if(!build_on_gpu && adypt_bvh_load(cfg.bvh_filename, &cfg.bvh, &bvh) != ADYPT_OK)
	{
		adypt_build_info info;
		if(adypt_bvh_build(scene, &cfg.bvh, &bvh, &info) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: bvh build failed: %s\n", adypt_host_last_error()); return 1; }
		printf("[SBVH]building lasted %.0f ms, %lld nodes, %lld references\n[WideBVH]built with %lld nodes (%.0f ms)\n", info.sbvh_ms,
			   (long long)info.sbvh_nodes, (long long)info.refs, (long long)info.wide_nodes, info.wide_ms);
		if(adypt_bvh_save(bvh, cfg.bvh_filename, &cfg.bvh) != ADYPT_OK) { fprintf(stderr, "[INSTANCE]Err: Unable to save bvh %s\n", cfg.bvh_filename); return 1; }
	}
	const void *nodes; const int32_t *idx;
	adypt_scene_desc d;
	memset(&d, 0, sizeof(d));
	if(bvh)
	{
		d.n_nodes = adypt_bvh_nodes(bvh, &nodes); d.nodes = nodes;
		d.n_refs = adypt_bvh_tri_indices(bvh, &idx); d.tri_indices = idx;
	}
	d.triangles = tris; d.n_tris = n_tris; d.materials = mats; d.n_mats = n_mats;
	d.textures = (const adypt_texture *)tex; d.n_textures = n_tex;
	d.width = cfg.width; d.height = cfg.height; d.device = devices[0]; d.tile_rank = 0; d.tile_nranks = 1;
	// any number of devices through the library's multi-device boundary (one device is its n_dev = 1 case): tile rank i on devices[i], one gather per saved image
	adypt_multi *multi = nullptr;
	adypt_rebuild_info first_build;
	if((build_on_gpu ? adypt_create_multi_from_triangles(&multi, &d, devices.data(), (int)devices.size(), &cfg.bvh, policy.method, policy.radius, policy.split_budget, &first_build)
	                 : adypt_create_multi(&multi, &d, devices.data(), (int)devices.size())) != ADYPT_OK)
	{
		fprintf(stderr, "[TRACER]Err: %s\n", adypt_multi_last_error(nullptr));
		return 1;
	}
	auto err = [&]() { return adypt_multi_last_error(multi); };
	adypt_pt_params p;
	p.stack_size = cfg.stack_size; p.max_bounce = cfg.max_bounce; p.subpixel = cfg.subpixel; p.tmp_lifetime = cfg.tmp_lifetime;
	p.ray_tmin = cfg.ray_tmin; p.clamp = cfg.clamp; memcpy(p.sun, cfg.sun, 12); p.shift_seed = seed;
	float ip[16], iv[16];
	adypt_camera_matrices(cfg.fov, cfg.yaw, cfg.pitch, cfg.width, cfg.height, ip, iv);
	int r = adypt_multi_set_params(multi, &p);
	if(r == ADYPT_OK) r = adypt_multi_set_camera(multi, cfg.position, ip, iv);
	if(r == ADYPT_OK && sun_visibility) r = adypt_multi_set_sun_visibility(multi, 1, nullptr);
	if(r == ADYPT_OK) r = adypt_multi_set_instrumentation(multi, 1);
	if(r == ADYPT_OK && (until || denoise)) r = adypt_multi_set_noise_stats(multi, 1);
	if(r != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return 1; }
	// the figures of a rebuild that has just run: what the rebuild line prints
	auto rebuild_figures = [&](const adypt_rebuild_info &info) {
		float ms[7] = {0, 0, 0, 0, 0, 0, 0};
		(void)adypt_get_rebuild_timing(adypt_multi_context(multi, 0), ms, 7);
		std::string method = ploc ? "ploc radius " + std::to_string(ploc_radius) : "linear";
		if(have_split_budget)
		{
			int32_t presplit[2] = {-1, 0};
			(void)adypt_get_rebuild_presplit(adypt_multi_context(multi, 0), presplit);
			char text[64];
			snprintf(text, sizeof(text), " split budget %g level %d", split_budget, (int)presplit[0]);
			method += text;
		}
		char text[512];
		snprintf(text, sizeof(text), "%lld nodes, %lld references, %d levels, method %s, %.3f ms (keys %.3f, sort %.3f, tree %.3f, bottom-up %.3f, emission %.3f, Woop and nodes %.3f)", (long long)info.n_nodes,
		         (long long)info.n_refs, (int)info.levels, method.c_str(), ms[6], ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
		return std::string(text);
	};
	if(build_on_gpu) printf("[PT]BUILD: %s\n", rebuild_figures(first_build).c_str());
	// --pose / --part-matrices and the rebuild that goes with them: before the history poses, or with --follow-motion after them
	auto move_scene = [&]() -> bool {
	if(!pose.empty())
	{
		adypt_pose_outcome outcome;
		const int code = have_rebuild_above ? adypt_multi_update_triangles_auto(multi, 0, n_tris, pose_positions.data(), pose_normals.data(), &cfg.bvh, &policy, &outcome)
		                                    : adypt_multi_update_triangles(multi, 0, n_tris, pose_positions.data(), pose_normals.data());
		if(code != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return false; }
		float ms[4] = {0, 0, 0, 0};
		(void)adypt_get_refit_timing(adypt_multi_context(multi, 0), ms, 4);
		printf("[PT]INFO: pose %s: %lld triangles moved, refit %.3f ms (scatter %.3f, references and Woop %.3f, nodes %.3f)\n", pose.c_str(), (long long)n_tris, ms[3], ms[0], ms[1], ms[2]);
		if(have_rebuild_above)
			printf("[PT]INFO: pose policy: tree cost %.4f -> %.4f (ratio %.4f, allowed %g): %s\n", outcome.built.cost, outcome.refitted.cost, outcome.refitted.cost / outcome.built.cost, rebuild_above,
			       outcome.rebuilt ? ("rebuilt (" + rebuild_figures(outcome.rebuild) + ")").c_str() : "kept");
	}
	if(!part_matrices.empty() || morphing)
	{
		adypt_pose_outcome outcome;
		adypt_morph_binding layer;
		memset(&layer, 0, sizeof(layer));
		int code = adypt_multi_bind_parts(multi, part_of_triangle.data(), n_tris, n_parts);
		if(code == ADYPT_OK && morphing) code = adypt_multi_bind_morph(multi, morph_triangle.data(), morph_target.data(), morph_deltas.data(), (int64_t)morph_triangle.size(), (int32_t)morph_targets.size());
		if(code == ADYPT_OK && morphing) code = adypt_multi_get_morph_binding(multi, &layer);
		if(code == ADYPT_OK)
			code = morphing ? adypt_multi_pose_morph(multi, part_matrix.data(), n_parts, morph_weights.data(), (int32_t)morph_weights.size(), &cfg.bvh, have_rebuild_above ? &policy : nullptr, &outcome)
			                : adypt_multi_pose(multi, part_matrix.data(), n_parts, &cfg.bvh, have_rebuild_above ? &policy : nullptr, &outcome);
		if(code != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return false; }
		float ms[4] = {0, 0, 0, 0};
		(void)adypt_get_refit_timing(adypt_multi_context(multi, 0), ms, 4);
		if(morphing) printf("[PT]MORPH: targets %d entries %lld triangles %lld of %lld\n", (int)layer.n_targets, (long long)layer.n_entries, (long long)layer.n_tris_touched, (long long)n_tris);
		if(part_matrices.empty()) printf("[PT]INFO: morph pose: refit %.3f ms (weights, matrices and pose %.3f, references and Woop %.3f, nodes %.3f)\n", ms[3], ms[0], ms[1], ms[2]);
		else printf("[PT]POSE: parts %d triangles %lld from %s, refit %.3f ms (matrices and pose %.3f, references and Woop %.3f, nodes %.3f)\n", (int)n_parts, (long long)n_tris, part_matrices.c_str(), ms[3],
		       ms[0], ms[1], ms[2]);
		if(have_rebuild_above)
			printf("[PT]INFO: pose policy: tree cost %.4f -> %.4f (ratio %.4f, allowed %g): %s\n", outcome.built.cost, outcome.refitted.cost, outcome.refitted.cost / outcome.built.cost, rebuild_above,
			       outcome.rebuilt ? ("rebuilt (" + rebuild_figures(outcome.rebuild) + ")").c_str() : "kept");
	}
	if(rebuild)
	{
		adypt_rebuild_info info;
		const int code = have_split_budget ? adypt_multi_rebuild_bvh_ploc_split(multi, &cfg.bvh, ploc_radius, split_budget, &info)
		                 : ploc            ? adypt_multi_rebuild_bvh_ploc(multi, &cfg.bvh, ploc_radius, &info)
		                                   : adypt_multi_rebuild_bvh(multi, &cfg.bvh, &info);
		if(code != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return false; }
		printf("[PT]INFO: rebuild: %s\n", rebuild_figures(info).c_str());
	}
	return true;
	};
	if(!follow_motion && !move_scene()) return 1;

	std::vector<float> rgb((size_t)cfg.width * cfg.height * 3, 0.0f);
	std::vector<uint8_t> rgba8;
	// SaveResult (OglPathTracer.cpp:199-212) + the window's picture; written to a temporary name first so that a reader of a
	// progressive render never sees a half-written file
	auto save = [&]() -> bool {
		if(adypt_multi_read_radiance(multi, rgb.data()) != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return false; }
		const std::string tmp = out + ".part";
		if(adypt_save_exr(tmp.c_str(), rgb.data(), cfg.width, cfg.height, fp16) != ADYPT_OK || rename(tmp.c_str(), out.c_str()) != 0) { fprintf(stderr, "[PT]ERR: %s\n", adypt_host_last_error()); return false; }
		if(!preview.empty())
		{
			rgba8.assign((size_t)cfg.width * cfg.height * 4, 0);
			if(adypt_multi_read_display(multi, rgba8.data()) != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return false; }
			const std::string ptmp = preview + ".part";
			if(adypt_save_png(ptmp.c_str(), rgba8.data(), cfg.width, cfg.height) != ADYPT_OK || rename(ptmp.c_str(), preview.c_str()) != 0) { fprintf(stderr, "[PT]ERR: %s\n", adypt_host_last_error()); return false; }
		}
		return true;
	};

	const adypt_denoise_params dp{denoise_levels, 4.0f, 0.1f};
	const adypt_temporal_params tp{(float)history_cap, 1};
	// a temporal call as the options ask for it
	auto temporal_call = [&]() -> int {
		if(rectify) return adypt_multi_denoise_temporal_rectified(multi, &dp, &tp, &rp, follow_motion ? 1 : 0);
		return follow_motion ? adypt_multi_denoise_temporal_motion(multi, &dp, &tp) : adypt_multi_denoise_temporal(multi, &dp, &tp);
	};
	// --history-from: every earlier pose is rendered and committed to the denoiser's history, each with a shift_seed of its own (an unchanged seed would
	// repeat the very same samples, which the history would count twice); then the main config's camera and seed, from 0 spp
	for(size_t k = 0; k < history_cfg.size() && r == ADYPT_OK; ++k)
	{
		const adypt_config &h = history_cfg[k];
		float hp[16], hv[16];
		adypt_camera_matrices(h.fov, h.yaw, h.pitch, cfg.width, cfg.height, hp, hv);
		p.shift_seed = seed + 1u + (unsigned)k;
		r = adypt_multi_reset(multi);
		if(r == ADYPT_OK) r = adypt_multi_set_params(multi, &p);
		if(r == ADYPT_OK) r = adypt_multi_set_camera(multi, h.position, hp, hv);
		if(r == ADYPT_OK) r = adypt_multi_trace_spp(multi, spp);
		if(r == ADYPT_OK) r = temporal_call();
		if(r == ADYPT_OK) printf("[PT]INFO: history pose %s: %d spp committed\n", history_from[k].c_str(), spp);
	}
	if(r != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return 1; }
	if(follow_motion && !move_scene()) return 1; // (the history holds the scene as loaded, with its snapshot; a pose leaves the tracer at 0 spp)
	if(!history_cfg.empty() && r == ADYPT_OK)
	{
		p.shift_seed = seed;
		r = adypt_multi_reset(multi);
		if(r == ADYPT_OK) r = adypt_multi_set_params(multi, &p);
		if(r == ADYPT_OK) r = adypt_multi_set_camera(multi, cfg.position, ip, iv);
	}
	if(r != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return 1; }
	// the sample count of every pixel from the devices' blocks (every block has one owner)
	auto pixel_spp = [&](std::vector<float> *count_of) -> bool {
		count_of->assign((size_t)cfg.width * cfg.height, 0.0f);
		const int blocks_x = (cfg.width + 31) / 32;
		for(size_t k = 0; k < devices.size(); ++k)
		{
			adypt_ctx *c = adypt_multi_context(multi, (int)k);
			const int64_t n = adypt_read_block_spp(c, nullptr, nullptr, 0);
			std::vector<int32_t> index((size_t)std::max<int64_t>(n, 0)), count(index.size());
			if(n < 0 || (n > 0 && adypt_read_block_spp(c, index.data(), count.data(), n) != n)) { fprintf(stderr, "[TRACER]Err: %s\n", adypt_last_error(c)); return false; }
			for(size_t b = 0; b < index.size(); ++b)
				for(int y = (index[b] / blocks_x) * 32; y < std::min(cfg.height, (index[b] / blocks_x + 1) * 32); ++y)
					for(int x = (index[b] % blocks_x) * 32; x < std::min(cfg.width, (index[b] % blocks_x + 1) * 32); ++x) (*count_of)[(size_t)y * cfg.width + x] = (float)count[b];
		}
		return true;
	};

	double t0 = now_ms(), t_save = 0.0;
	adypt_noise noise;
	memset(&noise, 0, sizeof(noise));
	adypt_adaptive adapt;
	memset(&adapt, 0, sizeof(adapt));
	if(adaptive)
	{
		r = adypt_multi_trace_adaptive(multi, noise_target, min_spp, spp, check_every, &adapt);
		noise = adapt.noise;
	}
	else if(until)
	{
		// to the noise target, --spp the cap.  With --save-every K the image is written whenever K more samples are in: the call is then capped at
		// the next multiple of K and taken up again (the noise is looked at every check_every samples from there).
		for(bool done = false; !done && r == ADYPT_OK;)
		{
			const int now = adypt_multi_get_spp(multi);
			const int cap = save_every > 0 ? std::min(spp, std::max(2, (now / save_every + 1) * save_every)) : spp;
			const int least = std::min(min_spp, cap);
			r = adypt_multi_trace_until(multi, noise_target, least, cap, check_every, &noise);
			if(r != ADYPT_OK) break;
			done = noise.spp >= spp || (noise.spp >= min_spp && noise.worst_block <= noise_target);
			if(!done)
			{
				const double ts = now_ms();
				if(!save()) return 1;
				t_save += now_ms() - ts;
				printf("[PT]INFO: %d spp saved to %s\n", noise.spp, out.c_str());
				fflush(stdout);
			}
		}
	}
	else if(primary >= 0) r = adypt_multi_trace_primary(multi, primary);
	else if(save_every <= 0 || save_every >= spp) r = adypt_multi_trace_spp(multi, spp);
	else
		for(int done = 0; done < spp && r == ADYPT_OK;)
		{
			const int n = std::min(save_every, spp - done);
			r = adypt_multi_trace_spp(multi, n);
			done += n;
			if(r == ADYPT_OK && done < spp)
			{
				const double ts = now_ms();
				if(!save()) return 1;
				t_save += now_ms() - ts;
				printf("[PT]INFO: %d spp saved to %s\n", done, out.c_str());
				fflush(stdout);
			}
		}
	double t1 = now_ms() - t_save;
	if(r != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return 1; }
	adypt_stats st;
	if(adypt_multi_get_stats(multi, &st) != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return 1; }
	printf("[PT]INFO: %d spp on %d GPU%s, %llu rays in %.1f ms wall (%.1f Mrays/s; traversal kernels %.1f ms, shade kernels %.1f ms)\n",
		   adypt_multi_get_spp(multi), (int)devices.size(), devices.size() > 1 ? "s" : "", (unsigned long long)st.rays, t1 - t0,
		   st.rays / ((t1 - t0) * 1e3), st.trace_ms, st.shade_ms);
	if(!save()) return 1;
	printf("[PT]INFO: Saved image to %s\n", out.c_str());
	if(!preview.empty()) printf("[PT]INFO: Saved preview to %s\n", preview.c_str());
	if(until)
	{
		if(!noise_out.empty())
		{
			std::vector<float> e((size_t)cfg.width * cfg.height, 0.0f), grey((size_t)cfg.width * cfg.height * 3);
			if(adypt_multi_read_noise(multi, e.data()) != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return 1; }
			for(size_t i = 0; i < e.size(); ++i) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = e[i];
			if(adypt_save_exr(noise_out.c_str(), grey.data(), cfg.width, cfg.height, 0) != ADYPT_OK) { fprintf(stderr, "[PT]ERR: %s\n", adypt_host_last_error()); return 1; }
			printf("[PT]INFO: Saved noise to %s\n", noise_out.c_str());
		}
		if(!spp_out.empty())
		{
			std::vector<float> count_of, grey((size_t)cfg.width * cfg.height * 3, 0.0f);
			if(!pixel_spp(&count_of)) return 1;
			for(size_t i = 0; i < count_of.size(); ++i) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = count_of[i];
			if(adypt_save_exr(spp_out.c_str(), grey.data(), cfg.width, cfg.height, 0) != ADYPT_OK) { fprintf(stderr, "[PT]ERR: %s\n", adypt_host_last_error()); return 1; }
			printf("[PT]INFO: Saved sample counts to %s\n", spp_out.c_str());
		}
		if(adaptive)
			printf("[PT]ADAPTIVE: spp %d frozen %d of %d pixel_samples %lld (uniform %lld) mean_noise %.9g worst_block %.9g worst_index %d (target %.9g)\n", noise.spp, adapt.blocks_frozen,
			       adapt.blocks, (long long)adapt.pixel_samples, (long long)noise.spp * (long long)cfg.width * (long long)cfg.height, noise.mean_noise, noise.worst_block, noise.worst_index, noise_target);
		else printf("[PT]NOISE: spp %d mean_noise %.9g worst_block %.9g worst_index %d (target %.9g)\n", noise.spp, noise.mean_noise, noise.worst_block, noise.worst_index, noise_target);
	}
	if(denoise)
	{
		std::vector<float> den((size_t)cfg.width * cfg.height * 3, 0.0f);
		if((temporal ? temporal_call() : adypt_multi_denoise(multi, &dp)) != ADYPT_OK || adypt_multi_read_denoised(multi, den.data()) != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return 1; }
		if(adypt_save_exr(denoise_out.c_str(), den.data(), cfg.width, cfg.height, fp16) != ADYPT_OK) { fprintf(stderr, "[PT]ERR: %s\n", adypt_host_last_error()); return 1; }
		printf("[PT]INFO: Saved denoised image (%d levels) to %s\n", denoise_levels, denoise_out.c_str());
		if(temporal)
		{
			// on the host from the read-backs: a hit pixel found history when its effective sample count is above its block's own
			std::vector<float> length((size_t)cfg.width * cfg.height, 0.0f), count_of;
			std::vector<uint8_t> hit(length.size(), 0);
			if(adypt_multi_read_denoise_history(multi, length.data()) != ADYPT_OK || adypt_multi_read_denoise_guides(multi, nullptr, nullptr, nullptr, hit.data()) != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return 1; }
			if(!pixel_spp(&count_of)) return 1;
			long long hits = 0, with_history = 0;
			double sum = 0.0;
			for(size_t i = 0; i < length.size(); ++i)
				if(hit[i]) { ++hits; sum += length[i]; if(length[i] > count_of[i]) ++with_history; }
			printf("[PT]TEMPORAL: history on %lld of %lld hit pixels, mean length %.3f", with_history, hits, hits ? sum / (double)hits : 0.0);
			if(follow_motion)
			{
				std::vector<uint8_t> moved(length.size(), 0);
				if(adypt_multi_read_denoise_motion(multi, nullptr, moved.data()) != ADYPT_OK) { fprintf(stderr, "\n[TRACER]Err: %s\n", err()); return 1; }
				printf(", moved %lld pixels", (long long)std::count(moved.begin(), moved.end(), (uint8_t)1));
			}
			std::vector<float> kept;
			if(rectify)
			{
				kept.assign(length.size(), 1.0f);
				if(adypt_multi_read_denoise_rectify(multi, kept.data()) != ADYPT_OK) { fprintf(stderr, "\n[TRACER]Err: %s\n", err()); return 1; }
				printf(", rectified %lld pixels", (long long)std::count_if(kept.begin(), kept.end(), [](float k) { return k < 1.0f; }));
			}
			printf("\n");
			if(!rectify_out.empty())
			{
				std::vector<float> grey(kept.size() * 3);
				for(size_t i = 0; i < kept.size(); ++i) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = kept[i];
				if(adypt_save_exr(rectify_out.c_str(), grey.data(), cfg.width, cfg.height, 0) != ADYPT_OK) { fprintf(stderr, "[PT]ERR: %s\n", adypt_host_last_error()); return 1; }
				printf("[PT]INFO: Saved kept history shares to %s\n", rectify_out.c_str());
			}
			if(!history_out.empty())
			{
				std::vector<float> grey(length.size() * 3);
				for(size_t i = 0; i < length.size(); ++i) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = length[i];
				if(adypt_save_exr(history_out.c_str(), grey.data(), cfg.width, cfg.height, 0) != ADYPT_OK) { fprintf(stderr, "[PT]ERR: %s\n", adypt_host_last_error()); return 1; }
				printf("[PT]INFO: Saved history lengths to %s\n", history_out.c_str());
			}
		}
	}
	if(!guides_out.empty())
	{
		std::vector<float> g[3];
		for(auto &v : g) v.assign((size_t)cfg.width * cfg.height * 3, 0.0f);
		if(adypt_multi_read_denoise_guides(multi, g[0].data(), g[1].data(), g[2].data(), nullptr) != ADYPT_OK) { fprintf(stderr, "[TRACER]Err: %s\n", err()); return 1; }
		const char *const what[3] = {".albedo.exr", ".normal.exr", ".position.exr"};
		for(int k = 0; k < 3; ++k)
			if(adypt_save_exr((guides_out + what[k]).c_str(), g[k].data(), cfg.width, cfg.height, 0) != ADYPT_OK) { fprintf(stderr, "[PT]ERR: %s\n", adypt_host_last_error()); return 1; }
		printf("[PT]INFO: Saved guide images to %s.{albedo,normal,position}.exr\n", guides_out.c_str());
	}
	adypt_destroy_multi(multi);
	if(bvh) adypt_bvh_free(bvh);
	adypt_scene_free(scene);
	// like ~Instance (src/Instance.cpp:83-86): the config is written back on exit
	adypt_config_save(argv[1], &cfg);
	return 0;
}
