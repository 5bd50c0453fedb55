"""csrc/device/active_blocks.hpp holds adaptive sampling's host side — which owned 32x32 blocks a pass still traces, the freeze decision and THE loop
of adypt_trace_adaptive / adypt_multi_trace_adaptive — without HIP.  A driver compiled with g++ steps the loop over scripted block noise for 1 and 3
ranks and prints every call it makes; the freeze schedule, the active lists and slot maps, the steps and the result are checked against a simulation
written out here (not the header's expressions).  Also here: frame_plan.hpp's input for a cache image that a set change left stale."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")

DRIVER = r"""
#include "active_blocks.hpp"
#include <cstdio>
#include <map>
using namespace adypt;
// IN : w h nranks target min_spp max_spp check_every start_spp n_rows, then n_rows rows of one mean noise per image block (row k = the k-th read;
//      the last row repeats).  A frozen block keeps the noise it froze with.
// OUT: "T n | active blocks per rank" per trace call, "F spp | blocks" per freeze call followed by "A rank | active | slot" per rank,
//      "R code spp blocks frozen pixel_samples pixels mean worst index", "S traced frames per image block", "E error text"
int main()
{
	int w, h, nranks, min_spp, max_spp, every, start, n_rows;
	double target;
	while(scanf("%d %d %d %lf %d %d %d %d %d", &w, &h, &nranks, &target, &min_spp, &max_spp, &every, &start, &n_rows) == 9)
	{
		const int nbx = (w + 31) / 32, nby = (h + 31) / 32, nb = nbx * nby;
		std::vector<std::vector<double>> rows((size_t)n_rows, std::vector<double>((size_t)nb));
		for(auto &row : rows) for(double &v : row) if(scanf("%lf", &v) != 1) return 2;
		std::vector<ActiveBlocks> ranks((size_t)nranks);
		for(int r = 0; r < nranks; ++r) ranks[(size_t)r].reset(owned_blocks(w, h, r, nranks));
		std::vector<long long> traced((size_t)nb, start);
		std::map<int, double> kept; // the sum a frozen block froze with
		int counter = start, reads = 0;
		adypt_adaptive out;
		std::string error;
		const int rc = trace_adaptive("driver", &error, target, min_spp, max_spp, every, &out, [&] { return counter; },
			[&](int n) {
				printf("T %d |", n);
				for(const ActiveBlocks &ab : ranks) { printf(" %d", (int)ab.active.size()); for(int32_t b : ab.active) traced[(size_t)b] += n; }
				printf("\n");
				counter += n;
				return (int)ADYPT_OK;
			},
			[&](std::vector<BlockState> *blocks) {
				const std::vector<double> &row = rows[(size_t)std::min(reads, n_rows - 1)];
				++reads;
				blocks->clear();
				for(const ActiveBlocks &ab : ranks)
					for(size_t i = 0; i < ab.owned.size(); ++i)
					{
						const int b = ab.owned[i];
						const uint32_t count = (uint32_t)(std::min(32, w - (b % nbx) * 32) * std::min(32, h - (b / nbx) * 32));
						const bool frozen = ab.frozen_at[i] != 0;
						const double sum = frozen ? kept[b] : row[(size_t)b] * count;
						if(!frozen) kept[b] = sum;
						blocks->push_back(BlockState{b, sum, count, ab.spp_of(i, counter), frozen});
					}
				std::sort(blocks->begin(), blocks->end(), [](const BlockState &a, const BlockState &b) { return a.index < b.index; });
				return (int)ADYPT_OK;
			},
			[&](const std::vector<int32_t> &stop, int spp) {
				printf("F %d |", spp);
				for(int32_t b : stop) printf(" %d", b);
				printf("\n");
				for(int r = 0; r < nranks; ++r)
				{
					ActiveBlocks &ab = ranks[(size_t)r];
					ab.freeze(stop, spp);
					printf("A %d |", r);
					for(int32_t b : ab.active) printf(" %d", b);
					printf(" |");
					for(int32_t s : ab.slot) printf(" %d", s);
					printf(" | %lld\n", (long long)ab.active_image_px(w, h));
				}
				return (int)ADYPT_OK;
			});
		if(rc == ADYPT_OK)
			printf("R %d %d %d %d %lld %lld %.17g %.17g %d\n", rc, out.noise.spp, out.blocks, out.blocks_frozen, (long long)out.pixel_samples, (long long)out.noise.pixels, out.noise.mean_noise,
			       out.noise.worst_block, out.noise.worst_index);
		else printf("R %d %d\n", rc, counter);
		printf("S");
		for(long long t : traced) printf(" %lld", t);
		printf("\nE %s\nEND\n", error.c_str());
	}
	return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("active_blocks")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I" + DEVICE, str(d / "driver.cpp"), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]  # (also: the header needs neither hipcc nor a HIP include)
    return exe


def run(exe, w, h, nranks, target, min_spp, max_spp, every, start, rows):
    text = "%d %d %d %r %d %d %d %d %d\n" % (w, h, nranks, float(target) if target == target else 0.0, min_spp, max_spp, every, start, len(rows))
    if target != target:
        text = text.replace(" 0.0 ", " nan ", 1)
    text += "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in rows)
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    assert lines[-1] == "END"
    return lines[:-1]


def geometry(w, h, nranks):
    nbx, nby = (w + 31) // 32, (h + 31) // 32
    owner = {by * nbx + bx: (bx + by) % nranks for by in range(nby) for bx in range(nbx)}  # the diagonal interleave, written out
    count = {by * nbx + bx: min(32, w - bx * 32) * min(32, h - by * 32) for by in range(nby) for bx in range(nbx)}
    return nbx * nby, owner, count


def simulate(w, h, nranks, target, min_spp, max_spp, every, start, rows):
    """The calls the loop must make and what it must report, from the semantics of the issue: steps of check_every cut at the cap; a read after
    every step from 2 spp on; from min_spp on every active block with mean <= target freezes; the end when nothing is active or at the cap."""
    nb, owner, count = geometry(w, h, nranks)
    frozen, kept, calls, counter, reads = {}, {}, [], start, 0
    while True:
        n = min(every, max_spp - counter)
        if n > 0:
            calls.append(("T", n, [sum(1 for b in range(nb) if owner[b] == r and b not in frozen) for r in range(nranks)]))
            counter += n
        none_active = False
        if counter >= 2:
            row = rows[min(reads, len(rows) - 1)]
            reads += 1
            for b in range(nb):
                if b not in frozen:
                    kept[b] = row[b] * count[b]
            stop = [b for b in range(nb) if b not in frozen and counter >= min_spp and kept[b] / count[b] <= target]
            if stop:
                for b in stop:
                    frozen[b] = counter
                lists = []
                for r in range(nranks):
                    owned = [b for b in range(nb) if owner[b] == r]
                    active = [b for b in owned if b not in frozen]
                    lists.append((active, [owned.index(b) for b in active], sum(count[b] for b in active)))
                calls.append(("F", counter, stop, lists))
            none_active = len(frozen) == nb
        if n <= 0 or counter >= max_spp or none_active:
            break
    spp_b = [frozen.get(b, counter) for b in range(nb)]
    total = 0.0
    for b in range(nb):  # ascending block index
        total += kept[b]
    means = [kept[b] / count[b] for b in range(nb)]
    worst = max(range(nb), key=lambda b: (means[b], -b))
    pixels = sum(count.values())
    assert pixels == w * h
    return dict(calls=calls, spp=counter, blocks=nb, frozen=len(frozen), pixel_samples=sum(count[b] * spp_b[b] for b in range(nb)), pixels=pixels,
                mean=total / pixels, worst=means[worst], worst_index=worst, spp_b=spp_b)


def parse(lines):
    calls, result, traced, error = [], None, None, None
    i = 0
    while i < len(lines):
        kind, _, rest = lines[i].partition(" ")
        if kind == "T":
            n, _, per_rank = rest.partition("|")
            calls.append(("T", int(n), [int(v) for v in per_rank.split()]))
        elif kind == "F":
            spp, _, stop = rest.partition("|")
            calls.append(("F", int(spp), [int(v) for v in stop.split()], []))
        elif kind == "A":
            _, active, slot, px = rest.split("|")
            calls[-1][3].append(([int(v) for v in active.split()], [int(v) for v in slot.split()], int(px)))
        elif kind == "R":
            result = rest.split()
        elif kind == "S":
            traced = [int(v) for v in rest.split()]
        elif kind == "E":
            error = rest
        i += 1
    return calls, result, traced, error


def check(exe, case, rows):
    want = simulate(*case, rows)
    calls, result, traced, error = parse(run(exe, *case, rows))
    try:
        assert calls == want["calls"]
        assert error == "" and int(result[0]) == 0
        assert [int(v) for v in result[1:6]] == [want["spp"], want["blocks"], want["frozen"], want["pixel_samples"], want["pixels"]]
        assert float(result[6]) == want["mean"] and float(result[7]) == want["worst"] and int(result[8]) == want["worst_index"]
        assert traced == want["spp_b"]  # the frames the trace calls gave every block = its sample count
        assert want["pixel_samples"] == sum(c * n for c, n in zip(geometry(*case[:3])[2].values(), traced))
    except AssertionError:
        print("case", case, "\nwant", want, "\ngot", calls, result, traced, error)
        raise
    return want


def decaying(nb, levels, n_rows):
    """row k: block b at levels[b] / sqrt(k + 1): every block converges, each at its own pace; a level of 0 is a block without noise"""
    return [[levels[b] / math.sqrt(k + 1.0) for b in range(nb)] for k in range(n_rows)]


#        w    h   ranks        (100 x 75: 4 x 3 blocks, partial blocks at the right and bottom edge; 64 x 36 on 4 ranks: rank 3 owns nothing)
SHAPES = [(100, 75, 1), (100, 75, 3), (64, 36, 4), (64, 36, 1), (160, 90, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%d-ranks" % s)
def test_freeze_schedule_lists_and_result(driver, shape):
    w, h, nranks = shape
    nb, owner, count = geometry(w, h, nranks)
    if nranks == 4:
        assert 3 not in owner.values()  # the shape reaches a rank that owns nothing
    levels = [0.0 if b % 3 == 2 else 0.1 + 0.07 * ((b * 5) % 7) for b in range(nb)]
    levels[1] = 10.0  # never converges: still active at the cap
    rows = decaying(nb, levels, 8)
    want = check(driver, (w, h, nranks, 0.1, 8, 64, 8, 0), rows)
    assert want["spp"] == 64 and want["spp_b"][1] == 64 and 0 < want["frozen"] < nb
    assert min(want["spp_b"]) == 8 and len(set(want["spp_b"])) >= 3  # some at the first eligible check, several freeze counts
    freezes = [c for c in want["calls"] if c[0] == "F"]
    assert len(freezes) >= 2
    for _, _, _, lists in freezes:
        for active, slot, _ in lists:
            assert active == sorted(active) and slot == sorted(slot) and len(active) == len(slot)  # ascending: a subsequence of the owned list


def test_min_spp_is_respected_and_the_loop_ends_when_all_are_frozen(driver):
    nb = 12
    rows = [[0.0] * nb]  # nothing has noise: everything freezes at the first eligible check
    want = check(driver, (100, 75, 3, 0.0, 12, 64, 8, 0), rows)
    assert want["spp"] == 16 and want["frozen"] == nb and want["spp_b"] == [16] * nb  # checks at 8 (below min_spp = 12) and 16
    assert [c[1] for c in want["calls"] if c[0] == "T"] == [8, 8]
    want = check(driver, (100, 75, 1, 1e30, 2, 64, 1, 0), rows)  # check_every 1: no read at 1 spp, the first at 2
    assert want["spp"] == 2 and want["frozen"] == nb
    assert want["pixel_samples"] == 2 * 100 * 75


def test_the_last_step_is_cut_to_the_cap(driver):
    nb = 12
    rows = [[1.0] * nb]  # nothing converges
    want = check(driver, (100, 75, 3, 0.1, 8, 20, 8, 0), rows)
    assert [c[1] for c in want["calls"]] == [8, 8, 4] and want["spp"] == 20 and want["frozen"] == 0 and want["pixel_samples"] == 20 * 100 * 75
    want = check(driver, (100, 75, 1, 0.1, 8, 20, 8, 5), rows)  # continues an accumulation at 5 spp: 13, 20
    assert [c[1] for c in want["calls"]] == [8, 7] and want["spp"] == 20
    want = check(driver, (100, 75, 1, 0.1, 8, 20, 8, 20), rows)  # at the cap already: nothing is traced, the blocks are read once
    assert want["calls"] == [] and want["spp"] == 20
    want = check(driver, (100, 75, 1, 2.0, 8, 20, 8, 20), rows)  # ... and may freeze there
    assert [c[0] for c in want["calls"]] == ["F"] and want["frozen"] == nb


@pytest.mark.parametrize("bad", [(0.1, 8, 64, 0), (0.1, 1, 64, 8), (0.1, 16, 8, 8), (0.1, 0, 0, 8), (float("nan"), 8, 64, 8)], ids=str)
def test_refused_arguments_trace_nothing(driver, bad):
    target, min_spp, max_spp, every = bad
    calls, result, traced, error = parse(run(driver, 100, 75, 3, target, min_spp, max_spp, every, 0, [[0.5] * 12]))
    assert calls == [] and traced == [0] * 12
    assert int(result[0]) == -1 and int(result[1]) == 0  # ADYPT_E_INVALID, the counter where it was
    assert error == "driver: needs check_every >= 1, 2 <= min_spp <= max_spp and a target that is a number"  # (the wording of trace_until)


def test_the_comparison_is_worst_blocks(driver):
    """sum / count <= target in binary64: a block exactly at the target freezes, one ulp above does not"""
    nb = 4
    t = 0.3
    rows = [[t, math.nextafter(t, 1.0), 0.0, 1.0]]
    want = check(driver, (64, 36, 1, t, 2, 4, 2, 0), rows)
    # (the driver hands over mean x count and the loop divides again: the cases are kept only where that round trip is exact)
    nb_, owner, count = geometry(64, 36, 1)
    assert all((rows[0][b] * count[b]) / count[b] == rows[0][b] for b in range(nb))
    assert want["spp_b"] == [2, 4, 2, 4]


# ---- frame_plan.hpp: the pass behind a set change re-traces the camera rays of the group it starts in ----

PLAN_DRIVER = r"""
#include "frame_plan.hpp"
#include <cstdio>
int main()
{
	adypt::PlanInput in{};
	in.pipeline = 1; in.single_fused = in.first_fused = in.fused_bounces = 1; in.max_bounce = 6; in.noise_stats = 1;
	long long px;
	while(scanf("%d %d %d %d %lld %d", &in.spp, &in.remaining, &in.frames_in_flight, &in.tmp_lifetime, &px, &in.cache_stale) == 6)
	{
		in.n_local_px = px;
		const adypt::PassPlan p = adypt::plan_pass(in);
		printf("%d %d %d %d %d %d %d %d\n", p.kind == adypt::PassPlan::Rolling, p.m, p.first_retrace, p.n_retrace, p.n_groups, p.stale_retrace, p.use_cache, p.as_batch);
	}
	return 0;
}
"""


def test_plan_pass_with_a_stale_cache(tmp_path):
    (tmp_path / "driver.cpp").write_text(PLAN_DRIVER)
    exe = str(tmp_path / "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + DEVICE, str(tmp_path / "driver.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    cases = [(spp, rem, fif, life, 3072, stale) for spp in (0, 3, 8, 9, 17) for rem in (1, 2, 6, 40) for fif in (1, 5, 128) for life in (1, 3, 4, 16) for stale in (0, 1)]
    text = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(cases)
    plans = {c: tuple(int(v) for v in line.split()) for c, line in zip(cases, out)}
    seen_stale = 0
    for (spp, rem, fif, life, px, stale), (rolling, m, first, n_retrace, n_groups, stale_retrace, use_cache, as_batch) in plans.items():
        fresh = plans[(spp, rem, fif, life, px, 0)]
        groups = sorted({(spp + k) // life for k in range(m)})
        assert n_groups == len(groups) and use_cache and as_batch
        if not stale or spp % life == 0:
            # nothing to repair (a pass that starts a group re-traces it anyway): the plan of today, which re-traces the frames with frame % life == 0
            assert (rolling, m, first, n_retrace, n_groups, 0, use_cache, as_batch) == fresh and not stale_retrace
            retraced = [k for k in range(m) if (spp + k) % life == 0]
            assert n_retrace == len(retraced) and (not retraced or first == retraced[0])
        else:
            # the camera pass runs batch frames 0, life, 2 life, ...: one per group the pass touches, the group it starts in included, and frame
            # g x life computes group g's sub-pixel index — (spp + g life) / life == spp / life + g
            seen_stale += 1
            assert stale_retrace and first == 0 and n_retrace == len(groups)
            assert [(spp + g * life) // life for g in range(n_retrace)] == groups
            assert (rolling, m, n_groups) == (fresh[0], fresh[1], fresh[4])  # the rest of the pass is what it was
    assert seen_stale > 20
