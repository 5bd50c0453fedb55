"""The device builder's walk over the tree (csrc/device/lbvh.hpp as build.hip uses it: Karras's node ids, bottom-up rows and counts, emission level by level
from a queue of items) run on the host by a small driver, under the address and undefined-behaviour sanitizers: its topology and reference order, refitted,
must be adypt_bvh_build_linear's bytes — the collapse's own pre-order walk and the device's level walk are two routes to one layout.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from adypt_amd import _native as N
from adypt_amd import api
from oracle import oracle_py as O
from tests import refit_truth as T
from tests.test_lbvh_definition import DEGENERATE, build_linear
from tests.test_refit_definition import lib_refit, rest, same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")

DRIVER = r"""
#include "lbvh.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace adypt;
// build.hip's BinTree over host vectors
struct Tree {
	int64_t n;
	std::vector<uint64_t> keys;
	std::vector<int32_t> left_, right_, parent;
	std::vector<RefitBox> boxes;
	std::vector<int> count;
	std::vector<CutRow> rows;
	std::vector<uint32_t> wb;
	int left(int i) const { return left_.at((size_t)i); }
	int right(int i) const { return right_.at((size_t)i); }
	const CutRow &row(int i) const { return rows.at((size_t)i); }
	uint32_t wide_below(int i) const { return wb.at((size_t)i); }
	bool is_leaf(int i) const { return (int64_t)i >= n - 1; }
	int32_t tri(int leaf) const { return (int32_t)(uint32_t)keys.at((size_t)(leaf - (n - 1))); }
	int tri_count(int i) const { return count.at((size_t)i); }
	void box(int i, float lo[3], float hi[3]) const { for(int k = 0; k < 3; ++k) { lo[k] = boxes.at((size_t)i).lo[k]; hi[k] = boxes.at((size_t)i).hi[k]; } }
};
// IN: triangles file (100-byte records), triangle_sah, node_sah, out prefix   OUT: <prefix>.nodes (80-byte records, box bytes zero), <prefix>.idx
int main(int argc, char **argv)
{
	if(argc != 5) return 2;
	FILE *f = fopen(argv[1], "rb");
	if(!f) return 2;
	std::vector<unsigned char> raw;
	unsigned char buf[4096];
	for(size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) raw.insert(raw.end(), buf, buf + k);
	fclose(f);
	const float tri_sah = (float)atof(argv[2]), node_sah = (float)atof(argv[3]);
	Tree t;
	t.n = (int64_t)(raw.size() / 100);
	const int64_t n = t.n;
	auto pos = [&](int64_t i, float p[9]) { memcpy(p, raw.data() + i * 100, 36); };
	RefitBox cb = refit_empty_box();
	for(int64_t i = 0; i < n; ++i) { float p[9]; pos(i, p); for(int k = 0; k < 3; ++k) { const float c = lbvh_centroid(p, k); cb.lo[k] = refit_min(cb.lo[k], c); cb.hi[k] = refit_max(cb.hi[k], c); } }
	t.keys.resize((size_t)n);
	for(int64_t i = 0; i < n; ++i) { float p[9]; pos(i, p); t.keys[(size_t)i] = lbvh_key(p, cb, (uint32_t)i); }
	std::sort(t.keys.begin(), t.keys.end());
	const size_t n_bin = (size_t)(2 * n - 1);
	t.left_.assign((size_t)(n - 1), -1); t.right_.assign((size_t)(n - 1), -1); t.parent.assign(n_bin, -1);
	for(int64_t i = 0; i + 1 < n; ++i)
	{
		int64_t first, last, split;
		lbvh_inner_node(t.keys.data(), n, i, &first, &last, &split);
		const int32_t l = lbvh_left_child(n, first, split), r = lbvh_right_child(n, last, split);
		t.left_[(size_t)i] = l; t.right_[(size_t)i] = r;
		t.parent.at((size_t)l) = (int32_t)i; t.parent.at((size_t)r) = (int32_t)i;
	}
	t.boxes.resize(n_bin); t.count.assign(n_bin, 0); t.rows.resize(n_bin); t.wb.assign(n_bin, 0);
	std::vector<int> arrived((size_t)std::max<int64_t>(n - 1, 1), 0);
	bool cost_ok = true;
	for(int64_t j = 0; j < n; ++j) // k_bottom_up, the leaves one after the other
	{
		const int leaf = (int)(n - 1 + j);
		float p[9]; pos(t.tri(leaf), p);
		t.boxes[(size_t)leaf] = refit_triangle_box(p);
		t.count[(size_t)leaf] = 1;
		cut_leaf_row(cut_area(t.boxes[(size_t)leaf].lo, t.boxes[(size_t)leaf].hi), tri_sah, t.rows[(size_t)leaf]);
		for(int cur = t.parent[(size_t)leaf]; cur >= 0; cur = t.parent[(size_t)cur])
		{
			if(arrived.at((size_t)cur)++ == 0) break;
			const int l = t.left(cur), r = t.right(cur);
			t.boxes[(size_t)cur] = refit_union(t.boxes[(size_t)l], t.boxes[(size_t)r]);
			t.count[(size_t)cur] = t.count[(size_t)r] + t.count[(size_t)l];
			CutRow row;
			cost_ok &= cut_inner_row(cut_area(t.boxes[(size_t)cur].lo, t.boxes[(size_t)cur].hi), t.count[(size_t)cur], tri_sah, node_sah, t.rows[(size_t)l], t.rows[(size_t)r], row);
			t.rows[(size_t)cur] = row;
			t.wb[(size_t)cur] = cut_wide_below(t, cur);
		}
	}
	if(!cost_ok) { printf("refused\n"); return 0; }
	const size_t n_nodes = std::max<uint32_t>(t.wb[0], 1u);
	std::vector<uint32_t> nodes(n_nodes * 20, 0u);
	std::vector<int32_t> idx((size_t)n, -1);
	std::vector<WideItem> items(1, WideItem{0, 0, 1u, 0u});
	int levels = 0;
	for(size_t begin = 0; begin < items.size(); ++levels) // k_emit, level by level; the next level is appended in REVERSED order: the queue's order must not show
	{
		const size_t end = items.size();
		std::vector<WideItem> next;
		for(size_t k = begin; k < end; ++k)
		{
			const WideItem it = items[k];
			if(it.w < 0 || (size_t)it.w >= n_nodes) { printf("layout\n"); return 0; }
			WideItem kids[8];
			const int nk = lbvh_emit_node(t, it, &nodes[(size_t)it.w * 20], idx.data(), (uint32_t)n, kids);
			for(int q = 0; q < nk; ++q) next.push_back(kids[q]);
		}
		std::reverse(next.begin(), next.end());
		items.insert(items.end(), next.begin(), next.end());
		begin = end;
	}
	if(items.size() != n_nodes) { printf("layout\n"); return 0; }
	std::string out = argv[4];
	f = fopen((out + ".nodes").c_str(), "wb"); fwrite(nodes.data(), 80, n_nodes, f); fclose(f);
	f = fopen((out + ".idx").c_str(), "wb"); fwrite(idx.data(), 4, idx.size(), f); fclose(f);
	printf("ok %zu %d\n", n_nodes, levels);
	return 0;
}
"""

CASES = {"tiny0": lambda: rest("tiny0")[0], "tiny1": lambda: rest("tiny1")[0], "tiny2": lambda: rest("tiny2")[0], "soup": lambda: T.soup(5000),
         "wave": lambda: T.wave(T.soup(5000))}
CASES.update(DEGENERATE)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ to compile the driver with")
    d = tmp_path_factory.mktemp("lbvh_walk")
    (d / "driver.cpp").write_text(DRIVER)
    exe = str(d / "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I" + DEVICE,
                        str(d / "driver.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]  # (also: the headers need neither hipcc nor a HIP include)
    return exe, d


@pytest.mark.parametrize("sah", [(0.3, 1.0), (1.0, 0.25)])
@pytest.mark.parametrize("what", sorted(CASES))
def test_level_walk_gives_the_collapse_bytes(what, sah, driver):
    exe, d = driver
    tris = CASES[what]()
    path = str(d / "tris.bin")
    np.ascontiguousarray(tris).view(np.uint8).tofile(path)
    out = subprocess.run([exe, path, repr(sah[0]), repr(sah[1]), str(d / "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    words = out.stdout.decode().split()
    assert words[0] == "ok", words
    nodes, idx = np.fromfile(str(d / "out.nodes"), dtype=np.uint8), np.fromfile(str(d / "out.idx"), dtype=np.int32)
    sc = api.Scene.FromArrays(tris, T.soup_material())
    b = api.WideBVH()
    cfg = api.InstanceConfig().bvh_params()
    cfg.triangle_sah, cfg.node_sah = sah
    b.BuildLinear(sc, cfg)
    assert int(words[1]) == len(b.nodes) // 80 and np.array_equal(idx, b.tri_indices)
    assert int(words[2]) == int(T.depths(np.ascontiguousarray(b.nodes).view(O.NODE_DT)).max()) + 1
    r, refitted = lib_refit(nodes, idx, tris)
    assert r == N.ADYPT_OK and same_bytes(refitted, b.nodes)


def test_costs_that_overflow_are_refused(driver):
    exe, d = driver
    tris = T.soup(300, 2)
    tris["p"] *= np.float32(1e19)  # areas of 1e40: every cost overflows
    path = str(d / "huge.bin")
    np.ascontiguousarray(tris).view(np.uint8).tofile(path)
    out = subprocess.run([exe, path, "0.3", "1.0", str(d / "huge")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-3000:]  # (and the sanitizers saw no stray access on the way)
    assert out.stdout.decode().split()[0] == "refused"
