// The command line of adypt_hip as one record.  parse_options fills it from argv, one option at a time; check_options refuses what does not go
// together and derives what the steps of main.cpp need.  Neither calls anything in the library, and after check_options nothing changes the record.
#pragma once
#include "adypt_hip.h"

#include <optional>
#include <string>
#include <vector>

// the one synopsis: what usage prints after the program's name (options.cpp describes every option above its table)
extern const char *const USAGE;

constexpr int GO_ON = -1; // what parse_options and check_options return when there is nothing to exit with

struct Options
{
	// as given
	std::string config;
	int spp = 64, fp16 = 0, primary = -1, sun_visibility = 0, save_every = 0;
	unsigned seed = 12345;
	std::string out = "result.exr", preview;
	std::vector<int> devices = {0};
	bool test_hooks = false;
	double noise_target = -1.0; // < 0: render to a fixed sample count
	int min_spp = 16, check_every = 16, adaptive = 0;
	std::string noise_out, spp_out, denoise_out, guides_out;
	int denoise_levels = 5;
	std::optional<int> denoise_specular; // --denoise-specular K: the guides follow mirrors and glass for K bounces
	std::optional<int> follow_specular;  // --follow-specular K: every temporal call follows them, and merges a followed pixel by its virtual point
	std::vector<std::string> history_from;
	std::string history_out;
	std::optional<double> history_cap; // 64 unless given
	bool follow_motion = false, rectify = false;
	bool rectify_detail = false; // one of --rectify-gamma, --rectify-radius, --rectify-out was given
	adypt_rectify_params rectify_params{3, 1.0f};
	std::string rectify_out;
	bool denoise_moments = false; // --denoise-moments: every temporal call is a moments call, from 1 spp
	std::string variance_out;
	std::optional<int> history_samples; // --history-samples T: the main render is traced by the history (adypt_multi_trace_by_history), --spp the cap
	int history_step = 4, history_tolerance = 31;
	bool history_plan_detail = false;   // one of --history-step, --history-tolerance, --reach-out, --plan-out was given
	std::string reach_out, plan_out;
	std::string pose, part_matrices;
	bool by_vertices = false, recompute_normals = false; // --pose by the mesh binding; its normals computed on the device
	std::vector<std::string> morph_targets;
	std::vector<float> morph_weights; // (a list that parses is never empty)
	bool bare_rebuild = false, build_on_gpu = false;
	std::optional<std::string> rebuild_method;
	std::optional<double> rebuild_above, split_budget;
	int ploc_radius = 8;
	std::string materials_from; // --materials-from other.obj: that scene's material table and textures, given to the context before the main render

	// derived by check_options
	bool until = false, denoise = false, temporal = false, morphing = false;
	bool ploc = false;    // the tree that --rebuild-method, --ploc-radius and --split-budget name: the first build of --build gpu, the policy's rebuild, or the rebuild asked for
	bool rebuild = false; // a rebuild outright, after the scene has moved
	adypt_pose_policy policy{0.0, 0, 8, 0.0};
};

// both return the exit code, or GO_ON
int parse_options(int argc, char **argv, Options *opt);
int check_options(Options *opt);
