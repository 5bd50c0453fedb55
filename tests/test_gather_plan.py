"""csrc/device/gather_plan.hpp decides the one exchange of the sharded frame — per-rank counts, the stride of the root's buffer and the sends and
receives a process posts — from plain numbers and without HIP.  A small driver compiled with g++ prints the plan for every choice of local ranks;
the plans are checked here against statements that are NOT the header's expressions: the counts against the library's exported shard geometry
(and a count of the diagonal interleave written out here), the operation lists against the three shapes the two callers of multi.hip rely on."""
import os
import shutil
import subprocess

import pytest

from adypt_amd import distributed as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
SHAPES = [(64, 36, 4), (100, 75, 3), (160, 96, 2), (1920, 1080, 8)]  # (64, 36, 4): 2 x 2 blocks, rank 3 owns none

DRIVER = r"""
#include "gather_plan.hpp"
#include <cstdio>
// IN: w h nranks n_local local...   OUT: counts... | stride | kind rank elements offset ...
int main()
{
	int w, h, n, k;
	while(scanf("%d %d %d %d", &w, &h, &n, &k) == 4)
	{
		std::vector<int> local((size_t)k);
		for(int &r : local) if(scanf("%d", &r) != 1) return 2;
		const adypt::GatherPlan p = adypt::plan_gather(w, h, n, local);
		for(long long c : p.counts) printf("%lld ", c);
		printf("| %lld |", (long long)p.stride);
		for(const adypt::GatherOp &op : p.ops) printf(" %c %d %lld %lld", op.kind == adypt::GatherOp::Send ? 'S' : 'R', op.rank, (long long)op.elements, (long long)op.offset);
		printf("\n");
	}
	return 0;
}
"""


def build_driver(tmp_path):
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + DEVICE, str(tmp_path / "driver.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]  # (also: the header needs neither hipcc nor a HIP include)
    return exe


def local_sets(nranks):
    """all local (adypt_multi), only rank 0 (the root process of adypt_comm_*), only rank k > 0 (a peer process)"""
    return [list(range(nranks)), [0]] + [[k] for k in range(1, nranks)]


def cases():
    return [(w, h, n, local) for (w, h, n) in SHAPES for local in local_sets(n)]


def run_driver(exe):
    text = "".join("%d %d %d %d %s\n" % (w, h, n, len(local), " ".join(map(str, local))) for (w, h, n, local) in cases())
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    plans = []
    for line in out.stdout.decode().splitlines():
        counts, stride, ops = line.split("|")
        ops = ops.split()
        plans.append(([int(c) for c in counts.split()], int(stride), [(ops[i], int(ops[i + 1]), int(ops[i + 2]), int(ops[i + 3])) for i in range(0, len(ops), 4)]))
    assert len(plans) == len(cases())
    return plans


def check(w, h, n, local, counts, stride, ops):
    # the counts: the library's shard geometry, and the diagonal interleave counted here
    nbx, nby = (w + 31) // 32, (h + 31) // 32
    assert counts == [D.block_count(w, h, r, n) * 1024 for r in range(n)]
    assert counts == [sum((bx + by) % n == r for by in range(nby) for bx in range(nbx)) * 1024 for r in range(n)]
    assert sum(counts) == nbx * nby * 1024
    assert stride == max([1024] + counts) and stride >= 1024
    senders = [r for r in range(1, n) if counts[r] > 0]
    if local == list(range(n)):     # one process owns every rank: Send1, Recv1, Send2, Recv2, ...
        want = [(kind, r) for r in senders for kind in "SR"]
    elif local == [0]:              # the root's process: Recv1, Recv2, ...
        want = [("R", r) for r in senders]
    else:                           # a peer's process: its one send, or nothing when it owns no block
        want = [("S", r) for r in local if r in senders]
    assert [(kind, r) for kind, r, _, _ in ops] == want
    for kind, r, elements, offset in ops:
        assert elements == 4 * counts[r] > 0 and offset == r * stride  # (a rank's send and the root's receive for it: the same count, from the same table)
        assert offset + counts[r] <= stride * n                        # ... and inside the root's buffer of stride x nranks
    assert all(counts[r] > 0 for _, r, _, _ in ops)                    # a rank that owns no block is in no operation


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")
def test_plans_for_every_choice_of_local_ranks(tmp_path):
    plans = run_driver(build_driver(tmp_path))
    empty = 0
    for (w, h, n, local), (counts, stride, ops) in zip(cases(), plans):
        try:
            check(w, h, n, local, counts, stride, ops)
        except AssertionError:
            print("case", (w, h, n, local), "plan", counts, stride, ops)
            raise
        empty += counts.count(0)
    assert empty > 0  # the shapes reach a rank without a block
    # the two sides of one exchange agree: what peer k's process sends is what the root's process receives from k
    by_case = {(w, h, n, tuple(local)): ops for (w, h, n, local), (_, _, ops) in zip(cases(), plans)}
    for (w, h, n) in SHAPES:
        sends = [op[1:] for k in range(1, n) for op in by_case[(w, h, n, (k,))]]
        assert sends == [op[1:] for op in by_case[(w, h, n, (0,))]]
        assert by_case[(w, h, n, tuple(range(n)))] == [op for s in sends for op in (("S",) + s, ("R",) + s)]
