// adypt_trace_until and adypt_multi_trace_until: THE loop and its argument check, over whatever traces (no HIP: a host compiler may include it,
// tests/test_noise_definition.py steps it over scripted noise values).
#pragma once
#include "../../../include/adypt_hip.h"

#include <algorithm>
#include <cstring>
#include <string>

namespace adypt {

// spp(): frames accumulated; trace(n): n more frames; read_noise(adypt_noise *): the image's numbers (asked only at 2 spp and more).  The two
// return ADYPT_OK or the code this returns.  Steps of check_every, the last one cut to reach max_spp exactly; after every step the noise is read,
// and the loop ends at max_spp, or from min_spp on once the worst block is at or below the target.  `fn` names the caller in *error, which is
// written only when the arguments are refused (nothing is traced then).
template <class Spp, class Trace, class ReadNoise>
int trace_until(const char *fn, std::string *error, double target, int min_spp, int max_spp, int check_every, adypt_noise *out, Spp spp, Trace trace, ReadNoise read_noise)
{
	if(check_every < 1 || min_spp < 2 || max_spp < min_spp || !(target == target))
	{
		*error = std::string(fn) + ": needs check_every >= 1, 2 <= min_spp <= max_spp and a target that is a number";
		return ADYPT_E_INVALID;
	}
	adypt_noise last;
	memset(&last, 0, sizeof(last));
	for(;;)
	{
		const int n = std::min(check_every, max_spp - spp());
		int r = n > 0 ? trace(n) : ADYPT_OK;
		if(r != ADYPT_OK) return r;
		const int now = spp();
		if(now >= 2 && (r = read_noise(&last)) != ADYPT_OK) return r;
		if(n <= 0 || now >= max_spp || (now >= min_spp && last.worst_block <= target)) break;
	}
	last.spp = spp();
	if(out) *out = last;
	return ADYPT_OK;
}

}  // namespace adypt
