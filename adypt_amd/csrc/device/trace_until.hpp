// THE stepping loop of adypt_trace_until, adypt_trace_adaptive and their adypt_multi_ forms, with its argument check, over whatever traces (no HIP:
// a host compiler may include it, tests/test_noise_definition.py and tests/test_active_blocks.py step it over scripted noise values).
#pragma once
#include "../../../include/adypt_hip.h"

#include <algorithm>
#include <cstring>
#include <string>

namespace adypt {

// spp(): frames accumulated; trace(n): n more frames; after_step(now, bool *finished): what the caller does with the image at `now` >= 2 frames (it is
// not asked below: one frame has no variance estimate), and whether the run is over.  The two return ADYPT_OK or the code this returns.  Steps of
// check_every, the last one cut to reach max_spp exactly; the loop ends when nothing is left to trace, at max_spp, or when after_step says finished.
// `fn` names the caller in *error, which is written only when the arguments are refused (nothing is traced then).  target and min_spp are only
// validated here — the rule is the same for every caller — and used by after_step.
template <class Spp, class Trace, class AfterStep>
int step_until(const char *fn, std::string *error, double target, int min_spp, int max_spp, int check_every, Spp spp, Trace trace, AfterStep after_step)
{
	if(check_every < 1 || min_spp < 2 || max_spp < min_spp || !(target == target))
	{
		*error = std::string(fn) + ": needs check_every >= 1, 2 <= min_spp <= max_spp and a target that is a number";
		return ADYPT_E_INVALID;
	}
	for(;;)
	{
		const int n = std::min(check_every, max_spp - spp());
		int r = n > 0 ? trace(n) : ADYPT_OK;
		if(r != ADYPT_OK) return r;
		const int now = spp();
		bool finished = false;
		if(now >= 2 && (r = after_step(now, &finished)) != ADYPT_OK) return r;
		if(n <= 0 || now >= max_spp || finished) return ADYPT_OK;
	}
}

// read_noise(adypt_noise *): the image's numbers.  After every step the noise is read, and the run is over from min_spp on once the worst block is at
// or below the target.
template <class Spp, class Trace, class ReadNoise>
int trace_until(const char *fn, std::string *error, double target, int min_spp, int max_spp, int check_every, adypt_noise *out, Spp spp, Trace trace, ReadNoise read_noise)
{
	adypt_noise last;
	memset(&last, 0, sizeof(last));
	const int r = step_until(fn, error, target, min_spp, max_spp, check_every, spp, trace, [&](int now, bool *finished) {
		const int rc = read_noise(&last);
		*finished = now >= min_spp && last.worst_block <= target;
		return rc;
	});
	if(r != ADYPT_OK) return r;
	last.spp = spp();
	if(out) *out = last;
	return ADYPT_OK;
}

}  // namespace adypt
