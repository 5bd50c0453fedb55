"""csrc/device/denoise_call.hpp makes every denoise call from the ABI structs in one place: the features of the entry's shape, the defaults, the refusal
and what follows from the features.  A small driver compiled with g++ makes the call of each of the seven entry shapes for a grid of arguments and
prints it; the lines are held here against rules written out below, which are NOT the header's expressions, and against the refusal texts as
denoise.hip spelled them before the header existed."""
import itertools
import math
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")

# the texts of denoise.hip's make_call, make_specular_call and make_virtual_call, behind their "<entry>: "
PARAMS = "levels must be in [1, 6], sigma_l and sigma_z positive numbers"
CAP = "history_cap must be a positive finite number"
RECTIFY = "the rectify radius must be in [1, 3], gamma a finite number that is not negative"
NULL = "specular is null"
BOUNCES = "bounces must be in [1, 8]"
NONE = "-"

# the seven shapes: (the entry, has history, takes rectify params, takes specular params, takes follow_motion, always follows motion, moments)
SHAPES = {"plain": ("adypt_denoise", False, False, False, False, False, False),
          "temporal": ("adypt_denoise_temporal", True, False, False, False, False, False),
          "motion": ("adypt_denoise_temporal_motion", True, False, False, False, True, False),
          "rectified": ("adypt_denoise_temporal_rectified", True, True, False, True, False, False),
          "moments": ("adypt_denoise_temporal_moments", True, False, False, True, False, True),
          "specular": ("adypt_denoise_specular", False, False, True, False, False, False),
          "temporal-specular": ("adypt_denoise_temporal_specular", True, False, True, False, False, False)}
ORDER = list(SHAPES)

# The driver's entries are denoise.hip's one-liners: the features each shape names, and the pointers its entry is given.
DRIVER = r"""
#include "denoise_call.hpp"
#include <cstdio>
#include <cstring>
using namespace adypt;
static float f32(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static unsigned u32(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static DenoiseCall entry(int shape, const char *fn, const adypt_denoise_params *p, const adypt_temporal_params *tp, const adypt_rectify_params *rp, const adypt_specular_params *sp, int follow_motion)
{
	switch(shape)
	{
	case 0: return make_call(fn, 0, p);
	case 1: return make_call(fn, kWithHistory, p, tp);
	case 2: return make_call(fn, kWithHistory | kWithMotion, p, tp);
	case 3: return make_call(fn, kWithHistory | kWithRectify | motion_if(follow_motion), p, tp, rp);
	case 4: return make_call(fn, kWithHistory | kWithMoments | motion_if(follow_motion), p, tp);
	case 5: return make_call(fn, kWithSpecular, p, nullptr, nullptr, sp);
	default: return make_call(fn, kWithHistory | kWithSpecular, p, tp, nullptr, sp);
	}
}
int main()
{
	char fn[64];
	int shape;
	while(scanf("%d %63s", &shape, fn) == 2)
	{
		int pg, levels, tg, commit, rg, radius, sg, bounces, fm;
		unsigned sl, sz, cap, gamma;
		if(scanf("%d %d %x %x %d %x %d %d %d %x %d %d %d", &pg, &levels, &sl, &sz, &tg, &cap, &commit, &rg, &radius, &gamma, &sg, &bounces, &fm) != 13) return 1;
		const adypt_denoise_params p{levels, f32(sl), f32(sz)};
		const adypt_temporal_params tp{f32(cap), commit};
		const adypt_rectify_params rp{radius, f32(gamma)};
		const adypt_specular_params sp{bounces};
		const DenoiseCall c = entry(shape, fn, pg ? &p : nullptr, tg ? &tp : nullptr, rg ? &rp : nullptr, sg ? &sp : nullptr, fm);
		if(c.fn != fn) return 2;
		const StageMarks m = c.marks();
		const HistoryKind k = c.kind();
		printf("%d %08x %08x %d %d %08x %d %d %d %08x %d %d %d %d %d %d %d %d %d|%s\n", c.prm.levels, u32(c.prm.sigma_l), u32(c.prm.sigma_z), (int)c.history, (int)c.motion, u32(c.history_cap),
		       (int)c.commit, (int)c.rectify, c.radius, u32(c.gamma), (int)c.moments, c.bounces, (int)c.virtual_point(), c.min_spp(), m.merge, m.first_level, (int)k.moments, k.followed,
		       (int)c.levels_read_merged(), c.refused.empty() ? "-" : c.refused.c_str());
	}
	return 0;
}
"""

# which call kind finds which history kind, and which sets of features there are
KINDS = r"""
#include "denoise_call.hpp"
#include <cstdio>
using namespace adypt;
int main()
{
	const adypt_specular_params one{1}, eight{8};
	const DenoiseCall calls[] = {make_call("t", kWithHistory, nullptr), make_call("m", kWithHistory | kWithMoments, nullptr), make_call("v1", kWithHistory | kWithSpecular, nullptr, nullptr, nullptr, &one),
	                             make_call("v8", kWithHistory | kWithSpecular, nullptr, nullptr, nullptr, &eight), make_call("tm", kWithHistory | kWithMotion, nullptr),
	                             make_call("r", kWithHistory | kWithRectify, nullptr), make_call("mm", kWithHistory | kWithMoments | kWithMotion, nullptr)};
	for(const DenoiseCall &reads : calls)
	{
		for(const DenoiseCall &left : calls) printf("%d", reads.kind() == left.kind() ? 1 : 0);
		printf("\n");
	}
	for(unsigned f = 0; f < 40; ++f) printf("%d", features_valid(f) ? 1 : 0);
	printf("\n%d %d %d %d %d %d\n", (int)kWithHistory, (int)kWithMotion, (int)kWithRectify, (int)kWithMoments, (int)kWithSpecular, kDenoiseTimingEvents);
	return 0;
}
"""

NAN, INF = 0x7fc00000, 0x7f800000


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def value(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


# (given, levels, sigma_l bits, sigma_z bits)
PARAM_CASES = [(0, 0, 0, 0), (1, 5, bits(4.0), bits(0.1)), (1, 0, bits(4.0), bits(0.1)), (1, 7, bits(4.0), bits(0.1)), (1, 5, bits(0.0), bits(0.1)), (1, 5, bits(-1.0), bits(0.1)),
               (1, 5, NAN, bits(0.1)), (1, 3, bits(2.0), bits(0.0)), (1, 6, bits(0.5), NAN)]
# (given, cap bits, commit)
CAP_CASES = [(0, 0, 0), (1, bits(64.0), 1), (1, bits(0.0), 1), (1, INF, 1), (1, NAN, 1), (1, bits(32.0), 0)]
# (given, radius, gamma bits)
RECTIFY_CASES = [(0, 0, 0), (1, 3, bits(1.0)), (1, 0, bits(1.0)), (1, 4, bits(1.0)), (1, 2, bits(-1.0)), (1, 1, INF)]
# (given, bounces)
SPECULAR_CASES = [(0, 0), (1, 0), (1, 1), (1, 8), (1, 9)]


def compile_and_run(tmp_path, name, source, text=""):
    (tmp_path / (name + ".cpp")).write_text(source)
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + DEVICE, str(tmp_path / (name + ".cpp")), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]  # (also: the header needs neither hipcc nor a HIP include)
    return subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()


def positive(b):
    return value(b) > 0.0  # (NaN is not)


def expected(shape, p, t, r, s, fm):
    """The call of a shape as the entries have always made it, and the first refusal in the order they have always checked in."""
    fn, history, takes_rp, takes_sp, takes_fm, always_motion, moments = SHAPES[shape]
    prm = p[1:] if p[0] else (5, bits(4.0), bits(0.1))
    cap, commit = (t[1], t[2]) if history and t[0] else (bits(64.0), 1 if history else 0)  # a call without history never commits
    radius, gamma = (r[1], r[2]) if takes_rp and r[0] else (3, bits(1.0))
    faults = []
    if not (1 <= prm[0] <= 6 and positive(prm[1]) and positive(prm[2])):
        faults.append(PARAMS)
    if history and not (positive(cap) and math.isfinite(value(cap))):
        faults.append(CAP)
    if takes_rp and not (1 <= radius <= 3 and value(gamma) >= 0.0 and math.isfinite(value(gamma))):
        faults.append(RECTIFY)
    if takes_sp and not s[0]:
        faults.append(NULL)
    if takes_sp and s[0] and not 1 <= s[1] <= 8:
        faults.append(BOUNCES)
    bounces = s[1] if takes_sp and not faults else 0  # (a refused call follows nothing)
    virtual = 1 if history and bounces > 0 else 0
    fields = (prm[0], prm[1], prm[2], int(history), int(always_motion or (takes_fm and fm == 1)), cap, commit, int(takes_rp), radius, gamma, int(moments), bounces, virtual,
              1 if moments else 2, 3 if history else 0, 4 if history else 3, int(moments), bounces if virtual else 0, int(history and not moments))
    return fields, (fn + ": " + faults[0]) if faults else NONE, len(faults)


def parse(line):
    head, reason = line.split("|", 1)
    f = head.split()
    hexed = (1, 2, 5, 9)
    return tuple(int(v, 16) if k in hexed else int(v) for k, v in enumerate(f)), reason


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")
def test_the_seven_shapes_over_the_grid(tmp_path):
    grid = list(itertools.product(PARAM_CASES, CAP_CASES, RECTIFY_CASES, SPECULAR_CASES, (0, 1)))
    cases = [(shape,) + g for shape in ORDER for g in grid]
    text = "".join("%d %s %d %d %x %x %d %x %d %d %d %x %d %d %d\n" % ((ORDER.index(shape), SHAPES[shape][0]) + p + t + r + s + (fm,)) for shape, p, t, r, s, fm in cases)
    out = compile_and_run(tmp_path, "driver", DRIVER, text)
    assert len(out) == len(cases)
    seen = {k: 0 for k in (PARAMS, CAP, RECTIFY, NULL, BOUNCES, NONE)}
    several = 0
    for case, line in zip(cases, out):
        want_fields, want_reason, n_faults = expected(*case)
        got_fields, got_reason = parse(line)
        assert got_reason == want_reason, (case, line)
        assert got_fields == want_fields, (case, line, want_fields)
        seen[want_reason.split(": ", 1)[-1]] += 1
        several += n_faults > 1
    assert all(seen.values()) and several > 0, seen
    # the rules once more, one at a time, as literal cases
    got = {case: parse(line) for case, line in zip(cases, out)}
    null_p, default_p, bad_p = PARAM_CASES[0], PARAM_CASES[1], PARAM_CASES[2]
    null_t, bad_t, kept_t = CAP_CASES[0], CAP_CASES[2], CAP_CASES[5]
    null_r, bad_r = RECTIFY_CASES[0], RECTIFY_CASES[2]
    null_s, bad_s, eight = SPECULAR_CASES[0], SPECULAR_CASES[4], SPECULAR_CASES[3]
    for shape in ORDER:
        fields, reason = got[(shape, null_p, null_t, null_r, eight, 0)]
        assert reason == NONE and fields[:3] == (5, 0x40800000, 0x3dcccccd), (shape, fields)                     # 5 / 4.0 / 0.1
        assert fields[5] == 0x42800000 and fields[8:10] == (3, 0x3f800000), (shape, fields)                          # cap 64; radius 3, gamma 1
        assert fields[6] == (0 if shape in ("plain", "specular") else 1), (shape, fields)                            # committing, but a call without history never
        assert fields[13] == (1 if shape == "moments" else 2), (shape, fields)                                       # min_spp
        assert fields[12] == (1 if shape == "temporal-specular" else 0), (shape, fields)                             # by the virtual point
        assert fields[14:16] == ((0, 3) if shape in ("plain", "specular") else (3, 4)), (shape, fields)              # the merge and first-level marks
        # every fault at once: the first in the order params, cap, rectify, specular
        assert got[(shape, bad_p, bad_t, bad_r, bad_s, 1)][1] == SHAPES[shape][0] + ": " + PARAMS
        assert got[(shape, null_p, kept_t, null_r, eight, 0)][0][5:7] == ((0x42000000, 0) if SHAPES[shape][1] else (0x42800000, 0)), shape  # the caller's cap and commit
    assert got[("plain", default_p, bad_t, bad_r, bad_s, 1)][1] == NONE                                              # what the entry is not given is not looked at
    assert got[("temporal", default_p, bad_t, bad_r, bad_s, 1)][1] == "adypt_denoise_temporal: " + CAP
    assert got[("rectified", default_p, bad_t, bad_r, bad_s, 1)][1] == "adypt_denoise_temporal_rectified: " + CAP
    assert got[("rectified", default_p, null_t, bad_r, bad_s, 1)][1] == "adypt_denoise_temporal_rectified: " + RECTIFY
    assert got[("moments", default_p, null_t, bad_r, bad_s, 1)][1] == NONE
    assert got[("specular", default_p, bad_t, bad_r, null_s, 0)][1] == "adypt_denoise_specular: " + NULL
    assert got[("specular", default_p, bad_t, bad_r, bad_s, 0)][1] == "adypt_denoise_specular: " + BOUNCES
    assert got[("temporal-specular", default_p, bad_t, null_r, null_s, 0)][1] == "adypt_denoise_temporal_specular: " + CAP
    assert got[("temporal-specular", default_p, null_t, bad_r, null_s, 0)][1] == "adypt_denoise_temporal_specular: " + NULL
    assert got[("temporal-specular", default_p, null_t, bad_r, eight, 0)][0][11:13] == (8, 1) and got[("specular", default_p, null_t, null_r, eight, 0)][0][11:13] == (8, 0)
    assert got[("rectified", default_p, null_t, null_r, null_s, 1)][0][4] == 1 and got[("rectified", default_p, null_t, null_r, null_s, 0)][0][4] == 0   # follow_motion
    assert got[("moments", default_p, null_t, null_r, null_s, 1)][0][4] == 1 and got[("temporal", default_p, null_t, null_r, null_s, 1)][0][4] == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")
def test_the_multi_entries_differ_in_name_only(tmp_path):
    bad_cap = (2, "adypt_multi_denoise_temporal_motion", PARAM_CASES[1], CAP_CASES[3], RECTIFY_CASES[0], SPECULAR_CASES[0], 0)
    bad_bounces = (6, "adypt_multi_denoise_temporal_specular", PARAM_CASES[0], CAP_CASES[0], RECTIFY_CASES[0], SPECULAR_CASES[1], 0)
    text = "".join("%d %s %d %d %x %x %d %x %d %d %d %x %d %d %d\n" % ((shape, fn) + p + t + r + s + (fm,)) for shape, fn, p, t, r, s, fm in (bad_cap, bad_bounces))
    out = compile_and_run(tmp_path, "driver", DRIVER, text)
    assert [parse(line)[1] for line in out] == ["adypt_multi_denoise_temporal_motion: " + CAP, "adypt_multi_denoise_temporal_specular: " + BOUNCES]
    assert parse(out[0])[0] == expected("motion", *bad_cap[2:])[0] and parse(out[1])[0] == expected("temporal-specular", *bad_bounces[2:])[0]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")
def test_history_kinds_and_feature_sets(tmp_path):
    out = compile_and_run(tmp_path, "kinds", KINDS)
    # rows: the call that reads; columns: the call that left the history.  plain-temporal, moments, by the virtual point with K = 1 and K = 8: only
    # equal kinds match (K = 1 does not find K = 8); motion and rectify change nothing about the kind
    #                 t  m  v1 v8 tm r  mm
    assert out[:7] == ["1000110",   # temporal
                       "0100001",   # moments
                       "0010000",   # virtual point, K = 1
                       "0001000",   # virtual point, K = 8
                       "1000110",   # motion
                       "1000110",   # rectified
                       "0100001"]   # moments with motion
    H, M, R, S2, SP = 1, 2, 4, 8, 16
    assert out[8] == "1 2 4 8 16 10"
    there_are = {0, H, H | M, H | R, H | R | M, H | S2, H | S2 | M, SP, H | SP}  # the seven shapes, two of them with and without follow_motion
    assert out[7] == "".join("1" if f in there_are else "0" for f in range(40))
    for f in (H | S2 | R, H | S2 | SP, H | SP | M, H | SP | R, M, R, S2, 32):  # moments + rectify, moments + bounces, bounces + motion, virtual + rectify, and history-less ones
        assert out[7][f] == "0", f
