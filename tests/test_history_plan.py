"""The integer half of history-aware sampling (csrc/device/history_reach.hpp), compiled with g++ and held against tests/history_reach_truth.py:
plan_block over scripted bins, the argument rule, and the calls trace_plan makes — for 1, 3 and 4 owners of the image's blocks, over
active_blocks.hpp's own state as adypt_trace_by_history and adypt_multi_trace_by_history run it.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import history_reach_truth as HT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")

DRIVER = r"""
#include "history_reach.hpp"
#include "active_blocks.hpp"
#include <cstdio>
using namespace adypt;
// IN, one request per line:
//   P target min_spp max_spp step tolerance b0 .. b64      -> "P want candidate"
//   V target min_spp max_spp step tolerance cap            -> "V 0|1"
//   T w h nranks start want_0 .. want_(blocks - 1)         -> "T n | active blocks per rank" per trace call, "F spp | blocks" per freeze call,
//                                                             then "S frames traced per block", "B sample count per block, as the owners hold it", "C counter"
int main()
{
	char kind;
	while(scanf(" %c", &kind) == 1)
	{
		if(kind == 'P')
		{
			int t, lo, hi, step, tol;
			uint32_t bins[kReachBins];
			if(scanf("%d %d %d %d %d", &t, &lo, &hi, &step, &tol) != 5) return 2;
			for(uint32_t &b : bins) if(scanf("%u", &b) != 1) return 2;
			const int want = plan_block(bins, t, lo, hi, step, tol);
			printf("P %d %d\n", want, plan_is_candidate(want, lo, hi, step) ? 1 : 0);
		}
		else if(kind == 'V')
		{
			int t, lo, hi, step, tol; float cap;
			if(scanf("%d %d %d %d %d %f", &t, &lo, &hi, &step, &tol, &cap) != 6) return 2;
			printf("V %d\n", plan_args_valid(t, lo, hi, step, tol, cap) ? 1 : 0);
		}
		else if(kind == 'T')
		{
			int w, h, nranks, start;
			if(scanf("%d %d %d %d", &w, &h, &nranks, &start) != 4) return 2;
			const int nb = ((w + 31) / 32) * ((h + 31) / 32);
			std::vector<std::pair<int32_t, int32_t>> wants;
			for(int b = 0; b < nb; ++b) { int v; if(scanf("%d", &v) != 1) return 2; wants.emplace_back(b, v); }
			std::vector<ActiveBlocks> ranks((size_t)nranks);
			for(int r = 0; r < nranks; ++r) ranks[(size_t)r].reset(owned_blocks(w, h, r, nranks));
			std::vector<long long> traced((size_t)nb, start);
			int counter = start;
			const int rc = trace_plan(wants, [&] { return counter; },
				[&](int n) {
					printf("T %d |", n);
					for(const ActiveBlocks &ab : ranks) { printf(" %d", (int)ab.active.size()); for(int32_t b : ab.active) traced[(size_t)b] += n; }
					printf("\n");
					counter += n;
					return 0;
				},
				[&](const std::vector<int32_t> &stop, int spp) {
					printf("F %d |", spp);
					for(int32_t b : stop) printf(" %d", b);
					printf("\n");
					for(ActiveBlocks &ab : ranks) ab.freeze(stop, spp);
					return 0;
				});
			if(rc != 0) return 3;
			printf("S");
			for(long long t : traced) printf(" %lld", t);
			std::vector<int> spp((size_t)nb, -1);
			for(const ActiveBlocks &ab : ranks) for(size_t i = 0; i < ab.owned.size(); ++i) spp[(size_t)ab.owned[i]] = ab.spp_of(i, counter);
			printf("\nB");
			for(int v : spp) printf(" %d", v);
			printf("\nC %d\n", counter);
		}
		else return 4;
	}
	return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("history_plan")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I" + DEVICE, str(d / "driver.cpp"), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]  # (also: the header needs neither hipcc nor a HIP include)
    return exe


def ask(exe, text):
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, (out.returncode, out.stderr.decode()[-2000:])
    return out.stdout.decode().splitlines()


def plan_block(exe, bins, target, min_spp=2, max_spp=64, step=4, tol=31):
    bins = list(bins) + [0] * (HT.BINS - len(bins))
    line, = ask(exe, "P %d %d %d %d %d %s\n" % (target, min_spp, max_spp, step, tol, " ".join(str(int(b)) for b in bins)))
    _, want, candidate = line.split()
    assert candidate == "1" and int(want) in HT.candidates(min_spp, max_spp, step), "every want is a candidate"
    assert int(want) == HT.plan_block(bins, target, min_spp, max_spp, step, tol), "the header and the truth disagree"
    return int(want)


def only(k, n=1024):
    """bins of a block whose n hit pixels all have the reach floor k"""
    b = [0] * HT.BINS
    b[k] = n
    return b


def test_no_history_gives_the_first_candidate_at_or_above_the_target(driver):
    assert plan_block(driver, only(0), 16) == 18                   # 2, 6, 10, 14, 18
    assert plan_block(driver, only(0), 16, step=7) == 16           # 2, 9, 16
    assert plan_block(driver, only(0), 16, min_spp=16) == 16
    assert plan_block(driver, only(0), 100) == 64                  # none reaches it: max_spp
    assert plan_block(driver, only(0), 64) == 64
    assert plan_block(driver, only(0), 1 << 20, max_spp=1 << 20, step=1 << 19) == 1 << 20  # (no overflow at the largest arguments)


def test_a_block_without_a_hit_pixel_gets_min_spp(driver):
    assert plan_block(driver, [], 16) == 2
    assert plan_block(driver, [], 16, min_spp=5, max_spp=9, tol=0) == 5


def test_history_shortens_the_count(driver):
    assert plan_block(driver, only(64), 16) == 2                   # the history alone is enough
    assert plan_block(driver, only(10), 16) == 6                   # 10 + 6 >= 16
    assert plan_block(driver, only(13), 16) == 6                   # 13 + 2 < 16
    assert plan_block(driver, only(14), 16) == 2
    assert plan_block(driver, only(63), 64) == 2 and plan_block(driver, only(64), 66) == 2 and plan_block(driver, only(64), 67) == 6


def test_max_spp_off_the_step_grid_is_the_last_candidate(driver):
    assert HT.candidates(2, 13, 4) == [2, 6, 10, 13]
    assert plan_block(driver, only(0), 12, max_spp=13) == 13       # 10 < 12: the next candidate is the cut one
    assert plan_block(driver, only(0), 13, max_spp=13) == 13
    assert plan_block(driver, only(0), 40, max_spp=13) == 13
    assert plan_block(driver, only(0), 5, min_spp=3, max_spp=3) == 3


def test_tolerance(driver):
    b = only(64, 1000)
    b[64], b[0] = 969, 31                                          # 31 of 1000 hit pixels without history
    assert plan_block(driver, b, 16, tol=31) == 2                  # allowed = 31: they may stay behind
    assert plan_block(driver, b, 16, tol=30) == 18                 # allowed = 30: one too many
    b[64], b[0] = 968, 32
    assert plan_block(driver, b, 16, tol=31) == 18                 # one pixel over
    assert plan_block(driver, b, 16, tol=32) == 2
    assert plan_block(driver, b, 16, tol=0) == 18
    assert plan_block(driver, only(0), 16, tol=999) == 18          # 999 permille of 1024 = 1022 < 1024
    one = only(0, 1)
    assert plan_block(driver, one, 16, tol=999) == 18              # allowed = 0 of one pixel
    mixed = only(0, 1)
    mixed[64] = 1023
    assert plan_block(driver, mixed, 16, tol=0) == 18 and plan_block(driver, mixed, 16, tol=1) == 2  # 1024 * 1 // 1000 = 1
    # allowed is an integer division: 999 hit pixels at 1 permille allow none
    few = only(64, 998)
    few[0] = 1
    assert plan_block(driver, few, 16, tol=1) == 18


def test_a_target_below_min_spp(driver):
    assert plan_block(driver, only(0), 1) == 2
    assert plan_block(driver, only(0), 3, min_spp=8, max_spp=16) == 8


def test_the_argument_rule(driver):
    cases = [(16, 2, 64, 4, 31, 64.0), (1, 2, 2, 1, 0, 1e-3), (1 << 20, 2, 64, 4, 999, 3.0e38), (0, 2, 64, 4, 31, 64.0), ((1 << 20) + 1, 2, 64, 4, 31, 64.0),
             (16, 1, 64, 4, 31, 64.0), (16, 8, 7, 4, 31, 64.0), (16, 2, 64, 0, 31, 64.0), (16, 2, 64, 4, -1, 64.0), (16, 2, 64, 4, 1000, 64.0),
             (16, 2, 64, 4, 31, 0.0), (16, 2, 64, 4, 31, -1.0), (16, 2, 64, 4, 31, float("inf")), (16, 2, 64, 4, 31, float("nan"))]
    lines = ask(driver, "".join("V %d %d %d %d %d %s\n" % (c[:5] + (repr(c[5]),)) for c in cases))
    assert [l.split()[1] == "1" for l in lines] == [HT.args_valid(*c) for c in cases]
    assert [HT.args_valid(*c) for c in cases] == [True] * 3 + [False] * 11


def geometry(w, h, nranks):
    nbx, nby = (w + 31) // 32, (h + 31) // 32
    return nbx * nby, {by * nbx + bx: (bx + by) % nranks for by in range(nby) for bx in range(nbx)}  # the diagonal interleave, written out


def trace(exe, w, h, nranks, want, start=0):
    lines = ask(exe, "T %d %d %d %d %s\n" % (w, h, nranks, start, " ".join(str(int(v)) for v in want)))
    calls = []
    for l in lines[:-3]:
        head, tail = l.split("|")
        kind, n = head.split()
        calls.append((kind, int(n), [int(v) for v in tail.split()]))
    traced, spp, counter = ([int(v) for v in l.split()[1:]] for l in lines[-3:])
    return calls, traced, spp, counter[0]


@pytest.mark.parametrize("nranks", [1, 3, 4])
def test_the_order_of_work(driver, nranks):
    w, h = 100, 75                      # 4 x 3 blocks
    nb, owner = geometry(w, h, nranks)
    want = [18, 2, 6, 18, 6, 6, 2, 10, 18, 2, 6, 10]
    calls, traced, spp, counter = trace(driver, w, h, nranks, want)
    # the truth's sequence: the distinct wants ascending, the blocks of each frozen at it, the largest group never
    expect, frozen = [], set()
    for step in HT.order_of_work(want):
        if step[0] == "T":
            expect.append(("T", step[1], [sum(1 for b in range(nb) if owner[b] == r and b not in frozen) for r in range(nranks)]))
        else:
            expect.append(("F", step[1], step[2]))
            frozen |= set(step[2])
    assert calls == expect
    assert [c[:2] for c in calls] == [("T", 2), ("F", 2), ("T", 4), ("F", 6), ("T", 4), ("F", 10), ("T", 8)]
    assert not any(kind == "F" and n == 18 for kind, n, _ in calls), "the largest group is never frozen"
    assert traced == want and spp == want and counter == 18, "every block was traced exactly as far as planned, and its owner says so"


def test_a_single_distinct_want_is_one_trace_and_no_freeze(driver):
    calls, traced, spp, counter = trace(driver, 100, 75, 3, [14] * 12)
    assert calls == [("T", 14, [4, 4, 4])] and traced == [14] * 12 and spp == [14] * 12 and counter == 14


def test_a_counter_already_at_the_largest_want_traces_nothing(driver):
    # (the entries refuse a counter that is not 0; the loop itself never traces a negative number of frames)
    calls, traced, _, counter = trace(driver, 64, 32, 1, [6, 6], start=6)
    assert calls == [] and traced == [6, 6] and counter == 6
