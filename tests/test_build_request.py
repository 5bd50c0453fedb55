"""csrc/device/build_request.hpp states once what every entry that builds a tree asks of the SAH costs, the method, the PLOC radius and the split
budget, and the defaults.  A small driver compiled with g++ prints the filled-in costs and the verdict of both checks for a grid of inputs; they are
held here against a table of rules that is NOT the header's expressions, and against the reason texts as the entry points spelled them before the
header existed."""
import itertools
import math
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")

# the texts of build.hip, geometry.hip, refit.hip, host/host_api.cpp and host/bvh_cost.cpp, behind their "who: "
SAH = "the SAH costs must be positive finite numbers"
METHOD = "method must be 0 (linear) or 1 (ploc)"
RADIUS = "the radius must be in [1, 32]"
BUDGET = "the split budget must be in [0, 1]"
NEEDS_PLOC = "a split budget needs method 1 (ploc)"
NONE = "-"

DRIVER = r"""
#include "build_request.hpp"
#include <cstdio>
#include <cstring>
static float f32(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static unsigned u32(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static double f64(unsigned long long u) { double d; memcpy(&d, &u, 8); return d; }
int main()
{
	char kind[8];
	while(scanf("%7s", kind) == 1)
	{
		const char *why = nullptr;
		if(kind[0] == 's') // sah <given> <triangle_sah bits> <node_sah bits>
		{
			int given; unsigned t, n;
			if(scanf("%d %x %x", &given, &t, &n) != 3) return 1;
			const adypt_bvh_params p{7, f32(t), f32(n)};
			const adypt_bvh_params cfg = adypt::build_cfg(given ? &p : nullptr);
			why = adypt::sah_refused(cfg);
			printf("%d %08x %08x ", (int)cfg.max_spatial_depth, u32(cfg.triangle_sah), u32(cfg.node_sah));
		}
		else // method <method> <radius> <budget bits>
		{
			int method, radius; unsigned long long b;
			if(scanf("%d %d %llx", &method, &radius, &b) != 3) return 1;
			why = adypt::method_refused(method, radius, f64(b));
			const adypt::BuildRequest q{adypt::build_cfg(nullptr), method, radius, f64(b)}, bad{adypt_bvh_params{0, 0.3f, -1.0f}, method, radius, f64(b)};
			if(adypt::request_refused(q) != why || adypt::request_refused(bad) != adypt::sah_refused(bad.cfg)) return 2; // both checks, the costs first
		}
		printf("%s\n", why ? why : "-");
	}
	return 0;
}
"""

# the three shapes of the fixed entries: what they set without a caller writing 0 or 1
SHAPES = r"""
#include "build_request.hpp"
#include <cstdio>
int main()
{
	const adypt_bvh_params p{3, 0.5f, 2.0f};
	const adypt::BuildRequest a = adypt::request_linear(nullptr), b = adypt::request_ploc(&p, 5), c = adypt::request_ploc(&p, 33, 0.25);
	printf("%d %d %g %g %g\n", a.method, a.radius, a.split_budget, a.cfg.triangle_sah, a.cfg.node_sah);
	printf("%d %d %g %g %g\n", b.method, b.radius, b.split_budget, b.cfg.triangle_sah, b.cfg.node_sah);
	printf("%d %d %g %g %g\n", c.method, c.radius, c.split_budget, c.cfg.triangle_sah, c.cfg.node_sah);
	printf("%d %d %s\n", adypt::kBuildLinear, adypt::kBuildPloc, adypt::kCutMax == 3.402823466e+38f ? "FLT_MAX" : "?");
	const adypt_bvh_params most{0, adypt::kCutMax, 1.0f}, more{0, 1.0f, adypt::refit_inf()}; // adypt_bvh_cost's bound is +inf: it takes FLT_MAX itself
	printf("%d %d %d\n", adypt::sah_refused(most) != nullptr, adypt::sah_refused(most, adypt::refit_inf()) == nullptr, adypt::sah_refused(more, adypt::refit_inf()) != nullptr);
	return 0;
}
"""

FLT_MAX_BITS = 0x7f7fffff
# (bits of a binary32, is it a cost the builders take): positive, and below FLT_MAX
COSTS = [(0xbf800000, False),        # -1
         (0x80000000, False),        # -0.0
         (0x00000000, False),        # 0
         (0x00000001, True),         # the smallest denormal
         (0x3e99999a, True),         # 0.3
         (0x3f800000, True),         # 1
         (FLT_MAX_BITS - 1, True),   # the largest finite number below FLT_MAX
         (FLT_MAX_BITS, False),      # FLT_MAX
         (0x7f800000, False),        # +inf
         (0x7fc00000, False)]        # NaN
METHODS = (-1, 0, 1, 2)
RADII = (-1, 0, 1, 8, 32, 33)
BUDGETS = [-1e-9, -0.0, 0.0, 1e-300, 0.25, 1.0, 1.0 + 2.0 ** -52, 1.5, math.inf, math.nan]


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def compile_and_run(tmp_path, name, source, text=""):
    (tmp_path / (name + ".cpp")).write_text(source)
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + DEVICE, str(tmp_path / (name + ".cpp")), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]  # (also: the header needs neither hipcc nor a HIP include)
    return subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()


def expected_method_reason(method, radius, budget):
    """The first fault in the order the entry points have always checked in: method, radius (ploc only), the budget's range, a budget without ploc."""
    faults = []
    if method not in (0, 1):
        faults.append(METHOD)
    if method == 1 and radius not in range(1, 33):
        faults.append(RADIUS)
    if math.isnan(budget) or budget < 0.0 or budget > 1.0:
        faults.append(BUDGET)
    if method == 0 and budget != 0.0:
        faults.append(NEEDS_PLOC)
    return faults[0] if faults else NONE


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")
def test_sah_costs_and_defaults_over_the_grid(tmp_path):
    cases = [(given, t, n) for given in (0, 1) for (t, _), (n, _) in itertools.product(COSTS, COSTS)]
    out = compile_and_run(tmp_path, "driver", DRIVER, "".join("sah %d %x %x\n" % c for c in cases))
    assert len(out) == len(cases)
    ok_of = dict(COSTS)
    seen = {SAH: 0, NONE: 0}
    for (given, t, n), line in zip(cases, out):
        depth, got_t, got_n, reason = line.split(" ", 3)
        if given:
            assert (int(depth), int(got_t, 16), int(got_n, 16)) == (7, t, n), (given, t, n, line)  # the caller's, bit for bit (NaN payload and -0.0 too)
            want = NONE if ok_of[t] and ok_of[n] else SAH
        else:
            assert (int(depth), int(got_t, 16), int(got_n, 16)) == (0, 0x3e99999a, 0x3f800000), line  # 0.3 / 1.0: InstanceConfig::BVH's defaults
            want = NONE
        assert reason == want, (given, hex(t), hex(n), line)
        seen[reason] += 1
    assert all(seen.values())


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")
def test_method_radius_and_budget_over_the_grid(tmp_path):
    cases = list(itertools.product(METHODS, RADII, BUDGETS))
    out = compile_and_run(tmp_path, "driver", DRIVER, "".join("method %d %d %x\n" % (m, r, f64_bits(b)) for m, r, b in cases))
    assert len(out) == len(cases)
    got = {(m, r, f64_bits(b)): line for (m, r, b), line in zip(cases, out)}
    seen = {k: 0 for k in (METHOD, RADIUS, BUDGET, NEEDS_PLOC, NONE)}
    for m, r, b in cases:
        line = got[(m, r, f64_bits(b))]
        assert line == expected_method_reason(m, r, b), (m, r, b, line)
        seen[line] += 1
    assert all(seen.values()), seen
    # the rules once more, one at a time, as literal cases
    at = lambda m, r, b: got[(m, r, f64_bits(b))]  # noqa: E731
    assert at(0, -1, 0.0) == at(0, 0, 0.0) == at(0, 33, 0.0) == NONE                       # the radius is not looked at for method 0
    assert at(1, 0, 0.0) == at(1, 33, 0.0) == at(1, -1, 0.25) == RADIUS and at(1, 1, 0.0) == at(1, 32, 1.0) == NONE
    assert at(1, 8, -0.0) == at(0, 8, -0.0) == NONE                                        # -0.0 is in [0, 1] and equals 0: no budget
    assert at(1, 8, 1e-300) == NONE and at(0, 8, 1e-300) == NEEDS_PLOC and at(0, 8, 1.0) == NEEDS_PLOC
    assert at(1, 8, -1e-9) == at(1, 8, 1.0 + 2.0 ** -52) == at(1, 8, math.inf) == at(1, 8, math.nan) == at(0, 8, math.nan) == BUDGET
    # several faults at once: the first in the order method, radius, range, needs-ploc
    assert at(2, 33, math.nan) == at(-1, 0, 1.5) == METHOD
    assert at(1, 33, math.nan) == at(1, 0, 1.5) == RADIUS
    assert at(0, 33, 1.5) == at(0, 0, math.inf) == BUDGET                                  # (out of range before "needs ploc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")
def test_the_shapes_of_the_fixed_entries(tmp_path):
    out = compile_and_run(tmp_path, "shapes", SHAPES)
    assert out == ["0 0 0 0.3 1", "1 5 0 0.5 2", "1 33 0.25 0.5 2", "0 1 FLT_MAX", "1 1 1"]  # (a constructor checks nothing: 33 is method_refused's to refuse)
