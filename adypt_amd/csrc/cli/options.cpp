// adypt_hip's options (the synopsis is USAGE below):
//   --build gpu: no .bvh cache is read or written and no tree is built on the host: the context is created from the triangles alone
//              (adypt_create_multi_from_triangles) and its first tree built on the GPU by --rebuild-method (ploc unless given), --ploc-radius and
//              --split-budget, which then name that build (and, with --rebuild-above, the policy's rebuild) instead of asking for a rebuild; one
//              [PT]BUILD: line reports it.  --pose and --rebuild-above work after it as they do otherwise; a bare --rebuild with it, or any other word than gpu (or host, the default), is exit 2
//   --pose moved.obj: the scene of the config (and its cached .bvh) with the vertices and normals of moved.obj — the same triangles in the same order,
//              moved — through adypt_multi_update_triangles: the BVH and the Woop data are refitted on the GPU, nothing is rebuilt
//   --by-vertices: with --pose only (else exit 2): the same pose by another road.  The scene as loaded is welded (adypt_weld_triangles) and bound as an
//              indexed mesh (adypt_multi_bind_mesh); vertex v takes its position and normal from moved.obj's corner at the place where v first appeared
//              in the weld, and the pose goes through adypt_multi_pose_vertices: 24 B per vertex cross the bus instead of 72 B per triangle.  A pose
//              that tears a vertex the scene shares — another corner of v has other position bits in moved.obj — is refused with one line naming the
//              vertex, exit 1.  --recompute-normals (with --by-vertices only, else exit 2): no normals are passed and the device computes smooth ones,
//              the only way to pose with an OBJ that carries none.  One [PT]MESH: line reports vertices, triangles, the largest valence and where
//              the normals came from.  --rebuild-above and --follow-motion act as with --pose
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
//   --materials-from other.obj: the other OBJ is loaded with the scene loader and the context is given ITS material table and textures
//              (adypt_multi_set_materials): the triangles keep their material ids, which now name the other table's entries, and are classified again.
//              With --history-from the swap comes after the history poses have been rendered and committed and before the main render: the history
//              shows the old light, the case --rectify is for.  One [PT]MATERIALS: line reports materials, textures and the triangles whose class
//              changed.  A file that cannot be opened, or the option given twice, is exit 2
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
//   --denoise-moments: with a temporal --denoise call only (else exit 2): every temporal call is a moments call (adypt_multi_denoise_temporal_moments) — the
//              history carries the second moment of the demodulated luminance, the variance is made after the merge (from a 7 x 7 window where the
//              history is shorter than 4 samples) — and --spp may be 1, for the --history-from poses too.  Combines with --follow-motion; not with
//              --rectify or --denoise-specular (exit 2).  The [PT]TEMPORAL: line then ends `, spatial variance on S pixels`: those that took the window
//              estimate.  --variance-out v.exr (needs --denoise-moments): the variance the first level saw, as a grey EXR
//   --denoise-specular K: with --denoise only, and with none of the temporal options (else exit 2): the guides of a pixel whose primary hit is a perfect
//              mirror or glass follow the reflection / transmission for up to K bounces, 1 .. 8, to the first surface that is neither
//              (adypt_multi_denoise_specular).  One [PT]SPECULAR: line reports the followed, escaped and truncated pixels and the rays
//   --follow-specular K: with a temporal --denoise call only (else exit 2): every temporal call, the --history-from poses included, is a followed one
//              (adypt_multi_denoise_temporal_specular): the guides of --denoise-specular K, and a pixel whose chain ended on a surface finds its history
//              through its virtual point.  Not with --denoise-specular, --follow-motion, --rectify or --denoise-moments (exit 2).  The [PT]TEMPORAL: line
//              then ends `, followed F pixels, H with history`; --guides-out writes the followed guides and PREFIX.chain.exr
//   --history-samples T: with a temporal --denoise call only (else exit 2): the main render, after the --history-from poses, is traced by the history
//              (adypt_multi_trace_by_history): before its first sample every pixel is asked how many samples of history the temporal call WILL find for it,
//              and every 32x32 block is traced to the smallest of 2, 2 + S, 2 + 2 S, ... (--history-step S, default 4; the last cut to --spp, which is
//              the cap) that brings all but P permille of its hit pixels (--history-tolerance P, 0 .. 999, default 31) to T samples, history and own
//              together.  T in 1 .. 1048576.  It follows --follow-motion and --denoise-moments, and takes --history-cap.  Not with --noise, --adaptive,
//              --save-every, --rectify or --follow-specular, and --spp must be at least 2 (exit 2).  The --history-from poses are rendered at --spp as
//              without it.  One line: [PT]PLAN: blocks B want W0..W1 pixel_samples N (uniform T*pixels) with_history H of P mean_reach L.
//              --reach-out reach.exr: the samples of history every pixel will find; --plan-out want.exr: every pixel's block's sample count; both grey
//              EXRs.  --history-step, --history-tolerance, --reach-out and --plan-out need --history-samples
//   --guides-out PREFIX: the feature images of the primary hit as PREFIX.albedo.exr, PREFIX.normal.exr and PREFIX.position.exr; with
//              --denoise-specular the followed guides, and the class code of every pixel as the grey PREFIX.chain.exr
#include "options.hpp"

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <limits>

const char *const USAGE =
	"scene.config [--spp N] [--out file.exr] [--fp16] [--primary TYPE] [--preview file.png] [--sun-visibility] [--seed S] [--device D | --devices D0,D1,...] "
	"[--save-every K] [--noise T [--min-spp N] [--check-every K] [--noise-out file.exr] [--adaptive [--spp-out file.exr]]] [--denoise file.exr [--denoise-levels L] [--denoise-specular K] "
	"[--history-from other.config]... [--history-cap C] [--history-out len.exr] [--follow-motion] [--rectify [--rectify-gamma G] [--rectify-radius R] "
	"[--rectify-out kept.exr]] [--denoise-moments [--variance-out v.exr]] [--follow-specular K] "
	"[--history-samples T [--history-step S] [--history-tolerance P] [--reach-out reach.exr] [--plan-out want.exr]]] [--guides-out PREFIX] [--pose moved.obj [--by-vertices [--recompute-normals]] | --part-matrices FILE] [--morph-target FILE.obj]... [--morph-weights w0,w1,...] [--rebuild] "
	"[--rebuild-method linear|ploc [--ploc-radius R] [--split-budget B]] [--rebuild-above R] [--build gpu] [--materials-from other.obj]";

// ---- values ----
// The whole of text as one number in [lo, hi]; else `<takes>, not <text>` on stderr and false.  An integer is read as one: 2.0 is not 2.
enum NumberKind { INTEGER, REAL };
static bool bounded_number(const char *text, NumberKind kind, double lo, double hi, const char *takes, double *value)
{
	char *end = nullptr;
	*value = kind == INTEGER ? (double)strtol(text, &end, 10) : strtod(text, &end);
	if(end != text && !*end && *value >= lo && *value <= hi) return true;
	fprintf(stderr, "%s, not %s\n", takes, text);
	return false;
}

// A comma-separated list of what item(q, &end) reads, which leaves end at q for what it does not take.  ends_on_comma: the list may end behind a
// comma, and may be empty.  false for anything else in text.
template <class T, class Item>
static bool comma_list(const char *text, bool ends_on_comma, Item item, std::vector<T> *list)
{
	list->clear();
	for(const char *q = text; *q || !ends_on_comma;)
	{
		char *end = nullptr;
		const T v = item(q, &end);
		if(end == q || (*end && *end != ',')) return false;
		list->push_back(v);
		if(!*end) break;
		q = end + 1;
	}
	return true;
}

// ---- the options: name, whether a value follows, what to do with it (false: refused, and said why) ----
// Most options store their value and leave judging it to check_options; numbers are read leniently (atoi, atof) unless the option says otherwise.
typedef bool (*Apply)(Options &o, const char *value);
template <bool Options::*M> static bool flag(Options &o, const char *) { o.*M = true; return true; }
template <int Options::*M> static bool int_flag(Options &o, const char *) { o.*M = 1; return true; }
template <int Options::*M> static bool lenient_int(Options &o, const char *v) { o.*M = atoi(v); return true; }
template <std::string Options::*M> static bool text(Options &o, const char *v) { o.*M = v; return true; }
template <std::vector<std::string> Options::*M> static bool one_more(Options &o, const char *v) { (o.*M).push_back(v); return true; }

static bool devices(Options &o, const char *v)
{
	const auto index = [](const char *q, char **end) { const long d = strtol(q, end, 10); if(d < 0) *end = (char *)q; return (int)d; };
	if(!comma_list(v, true, index, &o.devices)) { fprintf(stderr, "bad --devices list %s\n", v); return false; }
	if(o.devices.empty()) { fprintf(stderr, "empty --devices list\n"); return false; }
	return true;
}
static bool morph_weights(Options &o, const char *v)
{
	if(comma_list(v, false, strtof, &o.morph_weights)) return true;
	fprintf(stderr, "bad --morph-weights list %s\n", v);
	return false;
}
static bool history_cap(Options &o, const char *v)
{
	double cap;
	if(!bounded_number(v, REAL, std::numeric_limits<double>::denorm_min(), 3.0e38, "--history-cap takes a positive finite number", &cap)) return false;
	o.history_cap = cap;
	return true;
}
static bool rectify_radius(Options &o, const char *v)
{
	double radius;
	if(!bounded_number(v, INTEGER, 1, 3, "--rectify-radius takes 1, 2 or 3", &radius)) return false;
	o.rectify_params.radius = (int32_t)radius;
	return o.rectify_detail = true;
}
static bool rectify_gamma(Options &o, const char *v)
{
	double gamma;
	if(!bounded_number(v, REAL, 0.0, 3.0e38, "--rectify-gamma takes a finite number that is not negative", &gamma)) return false;
	o.rectify_params.gamma = (float)gamma;
	return o.rectify_detail = true;
}
static bool denoise_specular(Options &o, const char *v)
{
	double bounces;
	if(!bounded_number(v, INTEGER, 1, 8, "--denoise-specular takes a number of bounces from 1 to 8", &bounces)) return false;
	o.denoise_specular = (int)bounces;
	return true;
}
static bool follow_specular(Options &o, const char *v)
{
	double bounces;
	if(!bounded_number(v, INTEGER, 1, 8, "--follow-specular takes a number of bounces from 1 to 8", &bounces)) return false;
	o.follow_specular = (int)bounces;
	return true;
}
static bool history_samples(Options &o, const char *v)
{
	double target;
	if(!bounded_number(v, INTEGER, 1, 1 << 20, "--history-samples takes a number of samples from 1 to 1048576", &target)) return false;
	o.history_samples = (int)target;
	return true;
}
static bool history_step(Options &o, const char *v)
{
	double step;
	if(!bounded_number(v, INTEGER, 1, 1 << 20, "--history-step takes a number of samples from 1 to 1048576", &step)) return false;
	o.history_step = (int)step;
	return o.history_plan_detail = true;
}
static bool history_tolerance(Options &o, const char *v)
{
	double permille;
	if(!bounded_number(v, INTEGER, 0, 999, "--history-tolerance takes a number of permille from 0 to 999", &permille)) return false;
	o.history_tolerance = (int)permille;
	return o.history_plan_detail = true;
}
static bool rebuild_above(Options &o, const char *v)
{
	double ratio;
	if(!bounded_number(v, REAL, 0.0, DBL_MAX, "--rebuild-above takes a finite number >= 0", &ratio)) return false;
	o.rebuild_above = ratio;
	return true;
}
static bool build_where(Options &o, const char *v)
{
	const std::string where = v;
	if(where != "gpu" && where != "host") { fprintf(stderr, "--build is gpu or host, not %s\n", v); return false; }
	o.build_on_gpu = where == "gpu";
	return true;
}

static bool materials_from(Options &o, const char *v)
{
	if(!o.materials_from.empty()) { fprintf(stderr, "--materials-from is given twice: one table replaces the scene's\n"); return false; }
	if(!*v) { fprintf(stderr, "--materials-from takes the name of an OBJ file\n"); return false; }
	o.materials_from = v;
	return true;
}

static const struct Spec { const char *name; bool value; Apply apply; } SPECS[] = {
	{"--spp", true, lenient_int<&Options::spp>},
	{"--out", true, text<&Options::out>},
	{"--preview", true, text<&Options::preview>},
	{"--fp16", false, int_flag<&Options::fp16>},
	{"--sun-visibility", false, int_flag<&Options::sun_visibility>},
	{"--test-hooks", false, flag<&Options::test_hooks>}, // tests only: lets ADYPT_MULTI_SHARED_DEVICE put several shards on one device
	{"--primary", true, lenient_int<&Options::primary>},
	{"--seed", true, [](Options &o, const char *v) { o.seed = (unsigned)strtoul(v, nullptr, 10); return true; }},
	{"--device", true, [](Options &o, const char *v) { o.devices.assign(1, atoi(v)); return true; }},
	{"--devices", true, devices},
	{"--save-every", true, lenient_int<&Options::save_every>},
	{"--noise", true, [](Options &o, const char *v) { o.noise_target = atof(v); return true; }},
	{"--min-spp", true, lenient_int<&Options::min_spp>},
	{"--check-every", true, lenient_int<&Options::check_every>},
	{"--noise-out", true, text<&Options::noise_out>},
	{"--adaptive", false, int_flag<&Options::adaptive>},
	{"--spp-out", true, text<&Options::spp_out>},
	{"--denoise", true, text<&Options::denoise_out>},
	{"--denoise-levels", true, lenient_int<&Options::denoise_levels>},
	{"--denoise-specular", true, denoise_specular},
	{"--history-from", true, one_more<&Options::history_from>},
	{"--history-out", true, text<&Options::history_out>},
	{"--history-cap", true, history_cap},
	{"--follow-motion", false, flag<&Options::follow_motion>},
	{"--rectify", false, flag<&Options::rectify>},
	{"--rectify-out", true, [](Options &o, const char *v) { o.rectify_out = v; return o.rectify_detail = true; }},
	{"--rectify-radius", true, rectify_radius},
	{"--rectify-gamma", true, rectify_gamma},
	{"--denoise-moments", false, flag<&Options::denoise_moments>},
	{"--variance-out", true, text<&Options::variance_out>},
	{"--follow-specular", true, follow_specular},
	{"--history-samples", true, history_samples},
	{"--history-step", true, history_step},
	{"--history-tolerance", true, history_tolerance},
	{"--reach-out", true, [](Options &o, const char *v) { o.reach_out = v; return o.history_plan_detail = true; }},
	{"--plan-out", true, [](Options &o, const char *v) { o.plan_out = v; return o.history_plan_detail = true; }},
	{"--guides-out", true, text<&Options::guides_out>},
	{"--pose", true, text<&Options::pose>},
	{"--by-vertices", false, flag<&Options::by_vertices>},
	{"--recompute-normals", false, flag<&Options::recompute_normals>},
	{"--part-matrices", true, text<&Options::part_matrices>},
	{"--morph-target", true, one_more<&Options::morph_targets>},
	{"--morph-weights", true, morph_weights},
	{"--rebuild", false, flag<&Options::bare_rebuild>},
	{"--rebuild-above", true, rebuild_above},
	{"--rebuild-method", true, [](Options &o, const char *v) { o.rebuild_method = v; return true; }},
	{"--build", true, build_where},
	{"--ploc-radius", true, lenient_int<&Options::ploc_radius>},
	{"--materials-from", true, materials_from},
	{"--split-budget", true, [](Options &o, const char *v) { o.split_budget = atof(v); return true; }},
};

int parse_options(int argc, char **argv, Options *opt)
{
	if(argc < 2) { fprintf(stderr, "usage: %s %s\n", argv[0], USAGE); return 2; }
	opt->config = argv[1];
	for(int i = 2; i < argc; ++i)
	{
		const std::string a = argv[i];
		const Spec *spec = std::find_if(std::begin(SPECS), std::end(SPECS), [&](const Spec &s) { return a == s.name; });
		// (an option whose value is missing is not that option)
		if(spec == std::end(SPECS) || (spec->value && i + 1 >= argc)) { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
		if(!spec->apply(*opt, spec->value ? argv[++i] : nullptr)) return 2;
	}
	return GO_ON;
}

// ---- what does not go together, first refusal first; then what the steps read ----
static int refuse(const char *why)
{
	fprintf(stderr, "%s\n", why);
	return 2;
}

int check_options(Options *opt)
{
	Options &o = *opt;
	const bool above = o.rebuild_above.has_value();
	const std::string method = o.rebuild_method.value_or(o.build_on_gpu ? "ploc" : "linear");
	o.until = o.noise_target >= 0.0;
	o.morphing = !o.morph_targets.empty();
	o.denoise = !o.denoise_out.empty();
	o.temporal = !o.history_from.empty() || o.history_cap || !o.history_out.empty();

	if(o.build_on_gpu && o.bare_rebuild) return refuse("--build gpu has just built the tree: name its method with --rebuild-method, without --rebuild");
	if(method != "linear" && method != "ploc") return refuse("--rebuild-method is linear or ploc");
	if(o.split_budget && method != "ploc") return refuse("--split-budget needs --rebuild-method ploc");
	if(!o.pose.empty() && !o.part_matrices.empty()) return refuse("--pose and --part-matrices are two ways to move the scene: give one");
	if(o.by_vertices && o.pose.empty()) return refuse("--by-vertices needs --pose moved.obj");
	if(o.recompute_normals && !o.by_vertices) return refuse("--recompute-normals needs --pose moved.obj --by-vertices");
	if(o.morphing != !o.morph_weights.empty()) return refuse("--morph-target FILE.obj and --morph-weights w0,w1,... go together");
	if(o.morphing && o.morph_weights.size() != o.morph_targets.size()) { fprintf(stderr, "--morph-weights has %d weights for %d --morph-target\n", (int)o.morph_weights.size(), (int)o.morph_targets.size()); return 2; }
	if(o.morphing && !o.pose.empty()) return refuse("--morph-target morphs the scene as loaded: not together with --pose");
	if(above && o.pose.empty() && o.part_matrices.empty() && !o.morphing) return refuse("--rebuild-above needs --pose moved.obj, --part-matrices FILE or --morph-target");
	if(above && o.bare_rebuild) return refuse("--rebuild-above decides about the rebuild itself: name its method with --rebuild-method, without --rebuild");
	if(!o.until && !o.noise_out.empty()) return refuse("--noise-out needs --noise T");
	if(o.until && (o.primary >= 0 || o.spp < 2 || o.check_every < 1)) return refuse("--noise needs --spp >= 2, --check-every >= 1 and no --primary");
	if(o.adaptive && (!o.until || o.save_every > 0)) return refuse("--adaptive needs --noise T and does not combine with --save-every");
	if(!o.adaptive && !o.spp_out.empty()) return refuse("--spp-out needs --adaptive");
	if(!o.variance_out.empty() && !o.denoise_moments) return refuse("--variance-out needs --denoise-moments");
	if(o.denoise_moments && o.rectify) return refuse("--denoise-moments does not combine with --rectify: the clamp would leave the second moment inconsistent with the colour");
	if(o.denoise_moments && o.denoise_specular) return refuse("--denoise-moments does not combine with --denoise-specular");
	if(o.denoise_moments && !(o.denoise && o.temporal)) return refuse("--denoise-moments needs a temporal --denoise call: --denoise file.exr with --history-from, --history-cap or --history-out");
	if(o.denoise_moments && (o.primary >= 0 || o.spp < 1)) return refuse("--denoise with --denoise-moments needs --spp >= 1 and no --primary");
	if(o.denoise && !o.denoise_moments && (o.primary >= 0 || o.spp < 2)) return refuse("--denoise needs --spp >= 2 and no --primary");
	if(o.denoise && (o.denoise_levels < 1 || o.denoise_levels > 6)) return refuse("--denoise-levels must be in 1 .. 6");
	if(o.denoise_specular && !o.denoise) return refuse("--denoise-specular needs --denoise file.exr");
	if(o.denoise_specular && (o.temporal || o.follow_motion || o.rectify))
		return refuse("--denoise-specular has no temporal form: not together with --history-from, --history-cap, --history-out, --follow-motion or --rectify");
	if(o.temporal && !o.denoise) return refuse("--history-from, --history-cap and --history-out need --denoise file.exr");
	if(o.rectify_detail && !o.rectify) return refuse("--rectify-gamma, --rectify-radius and --rectify-out need --rectify");
	if(o.rectify && !o.temporal) return refuse("--rectify needs a temporal --denoise call: --denoise file.exr with --history-from, --history-cap or --history-out");
	if(o.follow_motion && !o.temporal) return refuse("--follow-motion needs a temporal --denoise call: --denoise file.exr with --history-from, --history-cap or --history-out");
	if(o.follow_specular && !(o.denoise && o.temporal)) return refuse("--follow-specular needs a temporal --denoise call: --denoise file.exr with --history-from, --history-cap or --history-out");
	if(o.follow_specular && (o.denoise_specular || o.follow_motion || o.rectify || o.denoise_moments))
		return refuse("--follow-specular does not combine with --denoise-specular, --follow-motion, --rectify or --denoise-moments");
	if(o.history_plan_detail && !o.history_samples) return refuse("--history-step, --history-tolerance, --reach-out and --plan-out need --history-samples T");
	if(o.history_samples && !(o.denoise && o.temporal)) return refuse("--history-samples needs a temporal --denoise call: --denoise file.exr with --history-from, --history-cap or --history-out");
	if(o.history_samples && (o.until || o.adaptive || o.save_every > 0)) return refuse("--history-samples plans the samples itself: not together with --noise, --adaptive or --save-every");
	if(o.history_samples && (o.rectify || o.follow_specular)) return refuse("--history-samples does not combine with --rectify or --follow-specular: the plan does not cover them");
	if(o.history_samples && o.spp < 2) return refuse("--history-samples needs --spp >= 2: no block stops below 2 samples");

	if(!o.materials_from.empty())
	{
		FILE *f = fopen(o.materials_from.c_str(), "rb");
		if(!f) { fprintf(stderr, "--materials-from %s: the file cannot be opened\n", o.materials_from.c_str()); return 2; }
		fclose(f);
	}

	// with --rebuild-above or --build gpu, --rebuild-method names the policy's rebuild or the first build; else naming a method asks for the rebuild
	o.rebuild = (o.bare_rebuild || o.rebuild_method) && !above && !o.build_on_gpu;
	o.ploc = method == "ploc";
	o.policy = adypt_pose_policy{o.rebuild_above.value_or(0.0), o.ploc ? 1 : 0, o.ploc_radius, o.split_budget.value_or(0.0)};
	if(o.until) o.min_spp = std::max(2, std::min(o.min_spp, o.spp));
	return GO_ON;
}
