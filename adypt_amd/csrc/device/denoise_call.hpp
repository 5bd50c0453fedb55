// One denoise call, made once from the ABI structs: which features it has, its parameters with their defaults, the refusal if there is one, and what
// follows from the features — the form by the virtual point, the samples it needs, where its stage marks stand, the kind of history it reads and
// leaves.  The fourteen denoise entries of denoise.hip differ only in the features they name.  No HIP needed (tests/test_denoise_call.py compiles it
// with a host compiler).  Not part of the C-ABI.
#pragma once
#include "guide_chain.hpp" // (temporal.hpp, and with it denoise.hpp, rectify.hpp and moments.hpp, come along)
#include "../../../include/adypt_hip.h"

#include <cassert>
#include <string>

namespace adypt {

// What a call can be asked for beyond the filter itself.  kWithHistory: the temporal merge; the next three need it.  kWithSpecular: the guides follow mirrors
// and glass — with kWithHistory that is the merge by the virtual point.
enum CallFeature : unsigned { kWithHistory = 1, kWithMotion = 2, kWithRectify = 4, kWithMoments = 8, kWithSpecular = 16 };
constexpr unsigned motion_if(int follow_motion) { return follow_motion ? (unsigned)kWithMotion : 0u; }
// THE combinations there are.  No moments with rectify (the clamp would move the colour and leave S inconsistent with it) or with followed guides;
// the virtual point neither follows moved geometry nor rectifies.
constexpr bool features_valid(unsigned f)
{
	return f < 32u && ((f & kWithHistory) || !(f & (kWithMotion | kWithRectify | kWithMoments))) && !((f & kWithMoments) && (f & (kWithRectify | kWithSpecular))) && !((f & kWithSpecular) && (f & (kWithMotion | kWithRectify)));
}
static_assert(features_valid(0) && features_valid(kWithHistory) && features_valid(kWithHistory | kWithMotion) && features_valid(kWithHistory | kWithRectify) && features_valid(kWithHistory | kWithRectify | kWithMotion) &&
              features_valid(kWithHistory | kWithMoments) && features_valid(kWithHistory | kWithMoments | kWithMotion) && features_valid(kWithSpecular) && features_valid(kWithHistory | kWithSpecular),
              "every shape an entry has");
static_assert(!features_valid(kWithHistory | kWithMoments | kWithRectify) && !features_valid(kWithHistory | kWithMoments | kWithSpecular) && !features_valid(kWithHistory | kWithSpecular | kWithMotion) &&
              !features_valid(kWithHistory | kWithSpecular | kWithRectify) && !features_valid(kWithMotion) && !features_valid(kWithRectify) && !features_valid(kWithMoments),
              "and what no entry can express");

// Which kind of call wrote a history: H0.w is S (a moments call) or V, and H1.w the class of a call by the virtual point with this many bounces (a
// truncated chain's class depends on them) or, 0, the hit flag.  A call finds only a history of its own kind.
struct HistoryKind { bool moments = false; int followed = 0; };
inline bool operator==(const HistoryKind &a, const HistoryKind &b) { return a.moments == b.moments && a.followed == b.followed; }

constexpr int kDenoiseTimingEvents = 4 + kDenoiseMaxLevels; // start, guides, prepare, (the temporal merge,) every level
// Where the marks of the stage timer stand in a run: 0 the start, 1 behind the guides (several devices: the upload), 2 behind prepare, then — with
// history only — one behind the merge (and the gather, the window and the variance kernel where the call has them), then one behind every level.
// Stage k lies between marks k, k + 1.
struct StageMarks { int merge, first_level; }; // merge 0: the run has no such stage
constexpr StageMarks stage_marks(bool with_history) { return with_history ? StageMarks{3, 4} : StageMarks{0, 3}; }

struct DenoiseCall {
	DenoiseParams prm;
	bool history, motion;
	float history_cap; bool commit;        // of a call with history; one without commits nothing
	bool rectify; int radius; float gamma; // rectify.hpp
	bool moments;                          // the variance comes from temporal luminance moments (moments.hpp)
	int bounces;                           // the guides follow mirrors and glass for this many bounces; 0: the primary hit's guides
	const char *fn;
	std::string refused;                   // why the arguments are refused; empty: they are not

	bool virtual_point() const { return history && bounces > 0; } // adypt_denoise_temporal_specular: the chain unfolds, the merge goes by the virtual point
	int min_spp() const { return moments ? 1 : 2; } // the samples every block has to hold: V0 of denoise_prepare is not defined below 2, S0 is from 1
	StageMarks marks() const { return stage_marks(history); }
	HistoryKind kind() const { return HistoryKind{moments, virtual_point() ? bounces : 0}; }
	// a moments call's first level reads X0, where the variance kernel wrote (D, V); every other call with history reads the merged image itself
	bool levels_read_merged() const { return history && !moments; }
};

// The call of the ABI structs (null: the defaults — 5 levels, 4.0, 0.1; cap 64, committing; radius 3, gamma 1).  tp is looked at with kWithHistory only,
// rp with kWithRectify, sp with kWithSpecular.  The refusals, the first that applies: the parameters, the cap, the rectify parameters, specular.
inline DenoiseCall make_call(const char *fn, unsigned features, const adypt_denoise_params *p, const adypt_temporal_params *tp = nullptr, const adypt_rectify_params *rp = nullptr,
                             const adypt_specular_params *sp = nullptr)
{
	assert(features_valid(features));
	const bool history = features & kWithHistory, specular = features & kWithSpecular;
	DenoiseCall call{p ? DenoiseParams{p->levels, p->sigma_l, p->sigma_z} : kDenoiseDefaults, history, (features & kWithMotion) != 0, kTemporalDefaultCap, history, (features & kWithRectify) != 0,
	                 kRectifyDefaultRadius, kRectifyDefaultGamma, (features & kWithMoments) != 0, 0, fn, {}};
	if(history && tp) { call.history_cap = tp->history_cap; call.commit = tp->commit != 0; }
	if(call.rectify && rp) { call.radius = rp->radius; call.gamma = rp->gamma; }
	const std::string who = std::string(fn) + ": ";
	if(!denoise_params_valid(call.prm)) call.refused = who + "levels must be in [1, " + std::to_string(kDenoiseMaxLevels) + "], sigma_l and sigma_z positive numbers";
	else if(history && !temporal_cap_valid(call.history_cap)) call.refused = who + "history_cap must be a positive finite number";
	else if(call.rectify && !rectify_params_valid(call.radius, call.gamma))
		call.refused = who + "the rectify radius must be in [1, " + std::to_string(kRectifyMaxRadius) + "], gamma a finite number that is not negative";
	else if(specular && !sp) call.refused = who + "specular is null";
	else if(specular && !chain_bounces_valid(sp->bounces)) call.refused = who + "bounces must be in [1, " + std::to_string(kChainMaxBounces) + "]";
	else if(specular) call.bounces = sp->bounces;
	return call;
}

}  // namespace adypt
