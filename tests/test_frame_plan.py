"""csrc/device/frame_plan.hpp decides which kernels a wavefront pass launches, from plain numbers and without HIP.  A small driver compiled with
g++ prints plan_pass for a grid of inputs; the plans are checked here against definitions that are NOT the header's expressions: the tmpLifetime
bookkeeping by counting frames, the frame hand-out and the cut into pipes by their invariants, and the pipeline choice by the implications the GPU
tests rely on (tests/test_gpu_fused_bounces.py) and by what the tunables' comments promise (adypt_ctx in csrc/device/context.hpp, tunables.hpp)."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
MAX_PATHS = 1 << 26      # the path word of k_path has 26 bits for the path id (path_limits.hpp)
SUN_MAX_BOUNCE = 31      # ... and the sun-visibility query rides as bounce index 31
IN = ("spp", "remaining", "lookahead", "frames_in_flight", "tmp_lifetime", "max_bounce", "pipeline", "single_fused", "first_fused", "fused_bounces",
      "sun_visibility", "n_local_px")
OUT = ("rolling", "m", "hand_out", "first_retrace", "n_retrace", "n_groups", "as_batch", "use_cache", "fused_first", "fused_bounces", "sun_query", "sun_queue",
       "n_pipes", "f0", "f1", "f2", "f3")

DRIVER = r"""
#include "frame_plan.hpp"
#include <cstdio>
int main()
{
	adypt::PlanInput in;
	long long px;
	while(scanf("%d %d %d %d %d %d %d %d %d %d %d %lld", &in.spp, &in.remaining, &in.lookahead, &in.frames_in_flight, &in.tmp_lifetime, &in.max_bounce, &in.pipeline,
	            &in.single_fused, &in.first_fused, &in.fused_bounces, &in.sun_visibility, &px) == 12)
	{
		in.n_local_px = px;
		const adypt::PassPlan p = adypt::plan_pass(in);
		printf("%d %d %d %d %d %d %d %d %d %d %d %d %d", p.kind == adypt::PassPlan::Rolling, p.m, p.hand_out, p.first_retrace, p.n_retrace, p.n_groups, p.as_batch, p.use_cache,
		       p.fused_first, p.fused_bounces, p.sun_query, p.sun_queue, p.n_pipes);
		for(int k = 0; k < adypt::kMaxPipes; ++k) printf(" %d", k < p.n_pipes ? p.frames_of_pipe[k] : 0);
		printf("\n");
	}
	return 0;
}
"""


def grid():
    """Every combination of the four switches x the edges: n_local_px at 2^26 and one above, per frame and per batch; maxBounce 31 / 32; tmpLifetime 1; batches
    that span three and more tmpLifetime groups (6 frames from spp 3 with tmpLifetime 4 or 2); `remaining` below, at and above frames_in_flight."""
    for flags, la, fif, life, spp, rem, mb, pipe in itertools.product(range(16), (0, 1), (1, 3, 6, 32), (1, 2, 4, 16), (0, 3, 16, 17), (1, 2, 6, 7, 40), (5, 31, 32), (1, 2, 4)):
        m = fif if la else min(rem, fif)
        for px in (1024, MAX_PATHS // m, MAX_PATHS // m + 1, MAX_PATHS, MAX_PATHS + 1):
            yield (spp, rem, la, fif, life, mb, pipe, flags & 1, (flags >> 1) & 1, (flags >> 2) & 1, (flags >> 3) & 1, px)


def run_driver(tmp_path, cases):
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + DEVICE, str(tmp_path / "driver.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]  # (also: the header needs neither hipcc nor a HIP include)
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(cases)
    return [dict(zip(OUT, map(int, line.split()))) for line in out]


def check(i, p, plan_of):
    """`i`: the input as a dict, `p`: its plan, `plan_of(**changes)`: the plan of the same input with some fields changed."""
    spp, life, m = i["spp"], i["tmp_lifetime"], p["m"]
    # frames traced / handed to the caller
    assert m == (i["frames_in_flight"] if i["lookahead"] else min(i["remaining"], i["frames_in_flight"]))
    assert p["hand_out"] == min(i["remaining"], m) >= 1
    # tmpLifetime bookkeeping, by counting
    retrace = [f - spp for f in range(spp, spp + m) if f % life == 0]
    assert p["n_retrace"] == len(retrace)
    if retrace:
        assert p["first_retrace"] == retrace[0]
    else:
        assert p["first_retrace"] >= m
    assert p["n_groups"] == len({f // life for f in range(spp, spp + m)})
    # the cut into pipes
    frames = [p["f0"], p["f1"], p["f2"], p["f3"]][:p["n_pipes"]]
    assert 1 <= p["n_pipes"] <= min(i["pipeline"], 4, m) and sum(frames) == m and max(frames) - min(frames) <= 1 and min(frames) >= 1
    assert frames == sorted(frames, reverse=True)  # (the longer sub-batches come first: frame order = pipe order)
    # what the GPU tests rely on
    paths = m * i["n_local_px"]
    if p["rolling"]:
        assert m == 1 and p["as_batch"] and p["fused_bounces"]
    assert p["as_batch"] == (m > 1 or p["rolling"])
    if p["fused_bounces"]:
        assert p["fused_first"] and p["n_pipes"] == 1 and paths <= MAX_PATHS and p["as_batch"]
    if p["fused_first"]:
        assert p["use_cache"] and p["as_batch"]
    assert p["use_cache"] == (p["as_batch"] or spp % life != 0)  # only the lone launch-per-bounce frame makes camera rays of its own
    if p["sun_query"]:
        assert i["sun_visibility"] and p["fused_bounces"] and i["max_bounce"] <= SUN_MAX_BOUNCE
    assert p["sun_query"] + p["sun_queue"] == i["sun_visibility"]  # the query is traced exactly one way
    if i["sun_visibility"] and p["fused_first"]:
        assert p["fused_bounces"]  # k_shade_first's queries are traced by k_path alone
    if p["n_pipes"] > 1:
        assert not p["fused_bounces"]
    if i["pipeline"] >= 2 and m > 1:
        assert p["n_pipes"] > 1 and not p["fused_bounces"] and not p["rolling"]
    # the tunables, as their comments name the pipelines
    if not i["fused_bounces"]:  # ADYPT_FUSED_BOUNCES=0: k_trace + k_shade per bounce
        assert not p["fused_bounces"] and not p["rolling"] and not p["sun_query"]
    if not i["first_fused"]:    # ADYPT_FIRST_FUSED=0: camera rays and bounce 0 as k_gen_primary + k_shade (and k_path has nothing to start from)
        assert not p["fused_first"] and not p["fused_bounces"] and not p["rolling"]
    if not i["single_fused"] and m == 1:  # ADYPT_SINGLE_FUSED=0: a single frame is gen -> [trace -> shade] x maxBounce, accumulating by itself
        assert not p["rolling"] and not p["as_batch"] and not p["fused_first"] and not p["fused_bounces"]
    if m > 1:                   # ... and says nothing about batches
        assert p == plan_of(single_fused=1 - i["single_fused"])
    # the other direction: with everything on, whatever fits k_path's path word takes the one-launch pipeline
    fits = paths <= MAX_PATHS and (not i["sun_visibility"] or i["max_bounce"] <= SUN_MAX_BOUNCE)
    if i["first_fused"] and i["fused_bounces"] and fits and p["n_pipes"] == 1 and (m > 1 or i["single_fused"]):
        assert p["fused_bounces"] and p["fused_first"] and p["rolling"] == (m == 1)
    if m > 1 and i["first_fused"] and not i["sun_visibility"]:
        assert p["fused_first"]  # the sub-batch pipeline starts from the cached primary hits too


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")
def test_plan_pass_over_the_grid(tmp_path):
    cases = list(grid())
    plans = run_driver(tmp_path, cases)
    by_input = dict(zip(cases, plans))
    seen = {"rolling": 0, "fused_batch": 0, "per_bounce": 0, "sun_query": 0, "sun_queue": 0, "three_groups": 0, "over_per_frame": 0, "over_per_batch": 0}
    for case, p in by_input.items():
        i = dict(zip(IN, case))

        def plan_of(**changes):
            return by_input[tuple({**i, **changes}[k] for k in IN)]
        try:
            check(i, p, plan_of)
        except AssertionError:
            print("input", i, "plan", p)
            raise
        seen["rolling"] += p["rolling"]
        seen["fused_batch"] += p["fused_bounces"] and not p["rolling"]
        seen["per_bounce"] += not p["fused_bounces"]
        seen["sun_query"] += p["sun_query"]
        seen["sun_queue"] += p["sun_queue"]
        seen["three_groups"] += p["n_groups"] == 3
        seen["over_per_frame"] += i["n_local_px"] > MAX_PATHS
        seen["over_per_batch"] += p["m"] > 1 and i["n_local_px"] <= MAX_PATHS < p["m"] * i["n_local_px"]
    assert all(seen.values()), seen  # the grid reaches every pipeline and every edge
