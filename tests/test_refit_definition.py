"""Moving geometry on the host: adypt_bvh_refit (csrc/device/refit.hpp + refit_plan.hpp) against the numpy restatement (tests/refit_truth.py), against the
builder, and against a BVH rebuilt from the moved triangles.  No GPU."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from adypt_amd import _native as N
from adypt_amd import api
from oracle import oracle_py as O
from tests import refit_truth as T
from tests.helpers import GOLDEN, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
SCENES = ("tiny0", "tiny1", "tiny2", "soup")
DEPTHS = (48, -1)
POSES = {"rest": lambda t: np.array(t), "wave": T.wave, "jitter": T.jitter}


@functools.lru_cache(maxsize=None)
def rest(name):
    """(triangles TRI_DT, materials MAT_DT) of the rest pose"""
    if name == "soup":
        return T.soup(20000), T.soup_material()
    return np.fromfile(os.path.join(GOLDEN, name + ".tris"), dtype=O.TRI_DT), np.fromfile(os.path.join(GOLDEN, name + ".mats"), dtype=O.MAT_DT)


def build(tris, mats, depth):
    sc = api.Scene.FromArrays(tris, mats)
    b = api.WideBVH()
    cfg = api.InstanceConfig().bvh_params()  # the default SAH costs
    cfg.max_spatial_depth = depth
    b.Build(sc, cfg)
    return sc, b


@functools.lru_cache(maxsize=None)
def built(name, depth):
    """(api.Scene, api.WideBVH) of the rest pose; shared and never written"""
    tris, mats = rest(name)
    return build(tris, mats, depth)


def lib_refit(nodes, tri_indices, tris):
    """adypt_bvh_refit on a copy: (code, nodes)"""
    out = np.array(np.ascontiguousarray(nodes).view(np.uint8).reshape(-1))
    idx = np.ascontiguousarray(tri_indices, dtype=np.int32)
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    r = N.lib.adypt_bvh_refit(out.ctypes.data, len(out) // 80, idx.ctypes.data, len(idx), t.ctypes.data, len(t) // 100)
    return r, out


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(b).view(np.uint8).reshape(-1))


@pytest.mark.parametrize("pose", sorted(POSES))
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", SCENES)
def test_library_equals_numpy(name, depth, pose):
    _, b = built(name, depth)
    moved = POSES[pose](rest(name)[0])
    r, got = lib_refit(b.nodes, b.tri_indices, moved)
    assert r == N.ADYPT_OK
    want, lo, _, slo, shi = T.refit(b.nodes, b.tri_indices, moved)
    assert same_bytes(got, want)
    assert T.slots_contain(got, lo, slo, shi)


@pytest.mark.parametrize("name", SCENES)
def test_unsplit_tree_reproduces_the_builder(name):
    _, b = built(name, -1)
    assert len(b.tri_indices) == len(rest(name)[0])  # -1 disables spatial splits: one reference per triangle
    r, got = lib_refit(b.nodes, b.tri_indices, rest(name)[0])
    assert r == N.ADYPT_OK and same_bytes(got, b.nodes)


def test_wrapper_refits_in_place_and_split_trees_grow():
    tris, mats = rest("tiny0")
    sc, b = build(tris, mats, 48)
    assert len(b.tri_indices) > len(tris)  # spatial splits: the refit bounds whole triangles, so boxes may only grow
    before = np.array(b.nodes)
    b.Refit(sc)
    assert same_bytes(b.nodes, lib_refit(before, b.tri_indices, tris)[1]) and not same_bytes(b.nodes, before)
    topo = lambda n: [np.ascontiguousarray(n).view(O.NODE_DT)[f] for f in ("meta", "imask", "child_base", "tri_base")]
    assert all(np.array_equal(x, y) for x, y in zip(topo(b.nodes), topo(before)))


@pytest.mark.parametrize("pose", ["wave", "jitter"])
@pytest.mark.parametrize("name", ["soup", "tiny0", "tiny1"])
def test_hits_are_those_of_a_rebuilt_tree(name, pose):
    tris, mats = rest(name)
    _, b = built(name, 48)
    moved = POSES[pose](tris)
    r, nodes = lib_refit(b.nodes, b.tri_indices, moved)
    assert r == N.ADYPT_OK
    _, lo, _, slo, shi = T.refit(b.nodes, b.tri_indices, moved)
    assert T.slots_contain(nodes, lo, slo, shi)
    refitted = O.Scene(nodes, b.tri_indices, moved, mats)
    _, rb = build(moved, mats, 48)
    rebuilt = O.Scene(rb.nodes, rb.tri_indices, moved, mats)
    rays = T.rays_in_box(moved, 50000)
    a, c = O.trace(refitted, rays), O.trace(rebuilt, rays)
    differ = (a["tri_id"] != c["tri_id"]) | (bits(a["t"]) != bits(c["t"]))
    print("%s %s: %d of %d rays differ; nodes per ray refitted %.2f rebuilt %.2f" % (name, pose, differ.sum(), len(rays), a["nodes"].mean(), c["nodes"].mean()))
    assert differ.sum() == 0
    assert (a["tri_id"] >= 0).any()


def flat_scene(n, seed, point=False):
    t = T.soup(n, seed)
    t["p"][..., 2] = 0.25         # an axis of zero extent
    if point:
        t["p"][...] = (1.5, -2.0, 0.25)
    return t


def test_edge_cases():
    mats = T.soup_material()
    for tris in (flat_scene(40, 1), flat_scene(40, 2, point=True), T.soup(1, 3)):
        _, b = build(T.soup(len(tris), 5), mats, -1)  # (a tree of the same size built from a proper pose, then moved into the degenerate one)
        r, got = lib_refit(b.nodes, b.tri_indices, tris)
        want = T.refit(b.nodes, b.tri_indices, tris)[0]
        assert r == N.ADYPT_OK and same_bytes(got, want)
        n = np.ascontiguousarray(got).view(O.NODE_DT)
        if len(tris) > 1:  # z has no extent: exponent byte 0 and quantised bytes 0 in every node
            occ = n["meta"] != 0
            assert (n["e"][:, 2] == 0).all() and (n["qloz"][occ] == 0).all() and (n["qhiz"][occ] == 0).all()
            assert (n["e"][:, :2] == 0).all() == bool((tris["p"] == tris["p"][0, 0]).all())  # ... and in x and y only where all is one point
    _, b = build(flat_scene(40, 2, point=True), mats, -1)  # built in the degenerate pose too
    assert same_bytes(lib_refit(b.nodes, b.tri_indices, flat_scene(40, 2, point=True))[1], b.nodes)
    # the one-triangle root: one node, one leaf of one reference
    _, b = build(T.soup(1, 3), mats, 48)
    assert len(b.nodes) == 80 and list(np.ascontiguousarray(b.nodes).view(O.NODE_DT)["meta"][0] >> 5).count(1) == 1
    assert same_bytes(lib_refit(b.nodes, b.tri_indices, T.soup(1, 3))[1], b.nodes)
    # leaves of 1, 2 and 3 references are all among the scenes the library is held against the restatement on
    seen = set()
    for name in SCENES:
        nodes = np.ascontiguousarray(built(name, 48)[1].nodes).view(O.NODE_DT)
        _, _, _, leaf, _, count = T.decode(nodes)
        seen |= set(count[leaf].tolist())
    assert seen == {1, 2, 3}


@pytest.mark.parametrize("name", ["tiny0", "soup"])
def test_poses_in_a_row(name):
    tris = rest(name)[0]
    for depth in DEPTHS:
        _, b = built(name, depth)
        pose_a, pose_b = T.wave(tris), T.jitter(tris)
        via_a = lib_refit(lib_refit(b.nodes, b.tri_indices, pose_a)[1], b.tri_indices, pose_b)[1]
        assert same_bytes(via_a, lib_refit(b.nodes, b.tri_indices, pose_b)[1])
        back = lib_refit(lib_refit(b.nodes, b.tri_indices, pose_a)[1], b.tri_indices, tris)[1]
        assert same_bytes(back, lib_refit(b.nodes, b.tri_indices, tris)[1])
        if depth == -1:
            assert same_bytes(back, b.nodes)  # back in the rest pose: the builder's bytes again


# ---- the plan (refit_plan.hpp) through a host compiler ----
DRIVER = r"""
#include "refit_plan.hpp"
#include <cstdio>
// IN: file n_refs   OUT: "ok" | depth of every node | per level: its nodes ;  or "refused <why>"
int main(int argc, char **argv)
{
	if(argc != 3) return 2;
	FILE *f = fopen(argv[1], "rb");
	if(!f) return 2;
	std::vector<unsigned char> nodes;
	unsigned char buf[4096];
	for(size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) nodes.insert(nodes.end(), buf, buf + k);
	fclose(f);
	adypt::RefitPlan p;
	std::string why;
	if(!adypt::plan_refit(nodes.data(), (long long)(nodes.size() / 80), atoll(argv[2]), &p, &why)) { printf("refused %s\n", why.c_str()); return 0; }
	printf("ok |");
	for(int d : p.depth) printf(" %d", d);
	for(int l = 0; l < p.levels(); ++l)
	{
		printf(" |");
		for(long long k = p.level_begin[(size_t)l]; k < p.level_begin[(size_t)l + 1]; ++k) printf(" %d", p.order[(size_t)k]);
	}
	printf("\n");
	return 0;
}
"""


def malformed(nodes):
    """name -> node array that is not one tree"""
    n = np.ascontiguousarray(nodes).view(O.NODE_DT).reshape(-1)
    _, inner, _, leaf, _, _ = T.decode(n)
    out = {}
    i = int(np.nonzero(inner.any(axis=1))[0][0])
    a = n.copy(); a["child_base"][i] = len(n) + 5; out["child index out of range"] = a
    j = int(np.nonzero(leaf.any(axis=1))[0][-1])
    a = n.copy(); a["tri_base"][j] = 0xfffffff0; out["reference range out of range"] = a
    i2 = int(np.nonzero(inner.sum(axis=1) >= 2)[0][0])
    s = np.nonzero(inner[i2])[0]
    a = n.copy(); a["meta"][i2][s[1]] = a["meta"][i2][s[0]]; out["reached twice"] = a   # two slots name one child (and their other child is orphaned)
    a = np.concatenate([n, n[-1:]]); out["not reached"] = a                               # a node no slot names
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")
def test_plan(tmp_path):
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + DEVICE, str(tmp_path / "driver.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]  # (also: the headers need neither hipcc nor a HIP include)

    def run(nodes, n_refs):
        path = str(tmp_path / "nodes.bin")
        np.ascontiguousarray(nodes).view(np.uint8).tofile(path)
        out = subprocess.run([exe, path, str(n_refs)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert out.returncode == 0, out.stderr.decode()[-3000:]
        return out.stdout.decode().strip()

    for name in SCENES:
        _, b = built(name, 48)
        nodes = np.ascontiguousarray(b.nodes).view(O.NODE_DT)
        parts = run(nodes, len(b.tri_indices)).split("|")
        assert parts[0].strip() == "ok"
        depth = np.array(parts[1].split(), dtype=np.int64)
        levels = [np.array(p.split(), dtype=np.int64) for p in parts[2:]]
        assert np.array_equal(depth, T.depths(nodes))
        assert sorted(np.concatenate(levels).tolist()) == list(range(len(nodes)))  # every node in exactly one level
        for d, l in enumerate(levels):
            assert (depth[l] == d).all() and len(l) > 0
        _, inner, child, _, _, _ = T.decode(nodes)
        parent = np.broadcast_to(np.arange(len(nodes))[:, None], inner.shape)
        assert (depth[child[inner]] > depth[parent[inner]]).all()                  # every child is deeper than its parent
    _, b = built("tiny0", 48)
    tris = rest("tiny0")[0]
    for what, bad in malformed(b.nodes).items():
        assert run(bad, len(b.tri_indices)).startswith("refused"), what
        r, got = lib_refit(bad, b.tri_indices, tris)
        assert r == N.E_INVALID and same_bytes(got, bad), what                     # refused, and nothing was written
    idx = np.array(b.tri_indices); idx[3] = len(tris)
    assert lib_refit(b.nodes, idx, tris)[0] == N.E_INVALID
