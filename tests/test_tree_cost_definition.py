"""The SAH cost of a tree from its quantised boxes (csrc/device/tree_cost.hpp): adypt_bvh_cost against the numpy restatement, integer for integer; the
fixed point of an unsplit tree; that the cost orders the work a ray does; what is refused; the header without HIP.  No GPU."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from adypt_amd import _native as N
from adypt_amd import api
from oracle import oracle_py as O
from tests import refit_truth as RT
from tests import tree_cost_truth as T
from tests.helpers import GOLDEN, golden_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")

BUILDERS = ("sbvh48", "sbvh-1", "linear", "ploc", "ploc_split")
POSES = {"wave": RT.wave, "jitter": RT.jitter, "apart": lambda t: T.apart(t, 0.25)}


def params(depth=0):
    cfg = api.InstanceConfig().bvh_params()  # the default SAH costs
    cfg.max_spatial_depth = depth
    return cfg


@functools.lru_cache(maxsize=None)
def soup():
    return RT.soup(5000), RT.soup_material()


def build(tris, mats, how):
    sc = api.Scene.FromArrays(tris, mats)
    b = api.WideBVH()
    if how == "sbvh48":
        b.Build(sc, params(48))
    elif how == "sbvh-1":
        b.Build(sc, params(-1))
    elif how == "linear":
        b.BuildLinear(sc, params())
    elif how == "ploc":
        b.BuildPLOC(sc, params())
    else:
        b.BuildPLOC(sc, params(), split_budget=0.3)
    return sc, b


@functools.lru_cache(maxsize=None)
def built(how):
    """(api.Scene, api.WideBVH) of soup(5000) in its rest pose; shared and never written"""
    return build(*soup(), how)


def lib_cost(nodes, cfg=None):
    """adypt_bvh_cost: (code, dict)"""
    n = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    out = N.TreeCost()
    r = N.lib.adypt_bvh_cost(n.ctypes.data, len(n) // 80, None if cfg is None else N.C.byref(cfg), N.C.byref(out))
    return r, out.as_dict()


def refitted(b, tris, mats):
    """a copy of the tree refitted to `tris`"""
    c = api.WideBVH()
    c.nodes, c.tri_indices = np.array(b.nodes), np.array(b.tri_indices)
    c.Refit(api.Scene.FromArrays(tris, mats))
    return c


def assert_same(nodes):
    r, got = lib_cost(nodes)
    assert r == N.ADYPT_OK, N.lib.adypt_host_last_error()
    want = T.cost(nodes)
    assert got == want, (got, want)
    assert got["inner_q"] > 0 or got["n_nodes"] == 1
    assert got["leaf_q"] > 0


@pytest.mark.parametrize("name", ["tiny0", "tiny1", "tiny2"])
def test_library_equals_numpy_on_the_golden_trees(name):
    _, _, nodes, _, _, _ = golden_scene(name)
    assert_same(nodes)


@pytest.mark.parametrize("how", BUILDERS)
def test_library_equals_numpy_as_built_and_refitted(how):
    tris, mats = soup()
    _, b = built(how)
    assert_same(b.nodes)
    for pose in sorted(POSES):
        assert_same(refitted(b, POSES[pose](tris), mats).nodes)


def test_wrapper_and_other_sah_costs():
    _, b = built("ploc")
    cfg = params()
    cfg.triangle_sah, cfg.node_sah = 0.7, 2.5
    got = b.Cost(cfg)
    assert got == T.cost(b.nodes, node_sah=2.5, triangle_sah=0.7)
    assert b.Cost() == T.cost(b.nodes) and b.Cost()["cost"] != got["cost"]


@pytest.mark.parametrize("how", ["sbvh-1", "linear", "ploc"])
def test_an_unsplit_tree_refitted_in_its_rest_pose_costs_what_it_cost(how):
    tris, mats = soup()
    _, b = built(how)
    assert len(b.tri_indices) == len(tris)
    assert refitted(b, tris, mats).Cost() == b.Cost()


def work(b, tris, mats, rays):
    h = O.trace(O.Scene(b.nodes, b.tri_indices, tris, mats), rays)
    return float(h["nodes"].mean()) + 0.3 * float(h["tris"].mean())


RATIOS = {0.05: 1.12, 0.25: 1.71, 1.5: 3.60}


def test_the_cost_orders_the_work_of_a_ray():
    """For soup(5000)'s PLOC tree moved apart by f = 0.05, 0.25 and 1.5 — refitted, and rebuilt for the pose — and for tiny1's tree with spatial splits
    refitted at rest: wherever two trees of one pose differ in cost by more than 25 %, the oracle's nodes + 0.3 tris per ray (20 000 rays) is ordered
    the same way; and the cost ratios are the recorded ones to two digits."""
    tris, mats = soup()
    _, b = built("ploc")
    c0 = b.Cost()["cost"]
    pairs = []
    for f, want in RATIOS.items():
        moved = T.apart(tris, f)
        rays = RT.rays_in_box(moved, 20000)
        kept = refitted(b, moved, mats)
        _, fresh = build(moved, mats, "ploc")
        ck, cf = kept.Cost()["cost"], fresh.Cost()["cost"]
        wk, wf = work(kept, moved, mats, rays), work(fresh, moved, mats, rays)
        print("f %.2f: ratio %.3f; refitted cost %.2f work %.2f (cost / work %.2f); rebuilt cost %.2f work %.2f" % (f, ck / c0, ck, wk, ck / wk, cf, wf))
        assert abs(ck / c0 - want) < 0.01
        pairs.append((ck, wk, cf, wf))
    t1, m1 = np.fromfile(os.path.join(GOLDEN, "tiny1.tris"), dtype=O.TRI_DT), np.fromfile(os.path.join(GOLDEN, "tiny1.mats"), dtype=O.MAT_DT)
    _, s = build(t1, m1, "sbvh48")
    assert len(s.tri_indices) > len(t1)  # (spatial splits)
    kept = refitted(s, t1, m1)
    rays = RT.rays_in_box(t1, 20000)
    cs, ck = s.Cost()["cost"], kept.Cost()["cost"]
    ws, wk = work(s, t1, m1, rays), work(kept, t1, m1, rays)
    print("tiny1 depth 48 at rest: ratio %.2f; built cost %.2f work %.2f; refitted cost %.2f work %.2f" % (ck / cs, cs, ws, ck, wk))
    assert abs(ck / cs - 10.5) < 0.05
    pairs.append((ck, wk, cs, ws))
    decided = 0
    for ca, wa, cb, wb in pairs:
        if max(ca, cb) > 1.25 * min(ca, cb):
            decided += 1
            assert (ca > cb) == (wa > wb), (ca, wa, cb, wb)
    assert decided >= 3


def test_refusals():
    _, _, nodes, _, _, _ = golden_scene("tiny0")
    out = N.TreeCost()
    n = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    assert N.lib.adypt_bvh_cost(n.ctypes.data, 0, None, N.C.byref(out)) == N.E_INVALID and N.lib.adypt_host_last_error()
    assert N.lib.adypt_bvh_cost(None, 1, None, N.C.byref(out)) == N.E_INVALID
    # a root without area: every triangle at one point
    tris, mats = RT.soup(40, 5), RT.soup_material()
    _, b = build(tris, mats, "sbvh-1")
    tris["p"][...] = np.float32(1.25)
    point = refitted(b, tris, mats)
    r, _ = lib_cost(point.nodes)
    assert r == N.E_INVALID and b"area" in N.lib.adypt_host_last_error()
    with pytest.raises(ValueError):
        T.sums(point.nodes)
    with pytest.raises(N.AdyptError):
        point.Cost()
    # SAH costs that are not positive finite numbers
    for ts, ns in ((0.0, 1.0), (0.3, -1.0), (float("nan"), 1.0), (0.3, float("inf"))):
        cfg = params()
        cfg.triangle_sah, cfg.node_sah = ts, ns
        r, _ = lib_cost(nodes, cfg)
        assert r == N.E_INVALID and b"SAH" in N.lib.adypt_host_last_error()
    # a slot of four times the root's area: a child's exponent bytes set 5 above the root's
    bad = np.array(np.ascontiguousarray(built("ploc")[1].nodes).view(O.NODE_DT).reshape(-1))
    bad["e"][1] = bad["e"][0] + 5
    r, _ = lib_cost(bad)
    assert r == N.E_INVALID and b"four times" in N.lib.adypt_host_last_error()
    with pytest.raises(ValueError):
        T.sums(bad)


DRIVER = r"""
#include "tree_cost.hpp"
#include <cstdio>
#include <cstring>
int main()
{
	unsigned char node[80];
	memset(node, 0, sizeof(node));
	node[adypt::kNodeExp] = node[adypt::kNodeExp + 1] = node[adypt::kNodeExp + 2] = 127; // scale 1
	node[adypt::kNodeMeta] = 0x20 | 0;                                                    // slot 0: a leaf of one reference
	for(int a = 3; a < 6; ++a) node[adypt::kNodeQuant + a * 8] = 2;                       // a box of 2 x 2 x 2
	uint32_t w[20], q[6], e[3];
	memcpy(w, node, 80);
	const float A = adypt::cost_root_area(w);
	adypt::cost_slot_bytes(node, 0, q, e);
	const adypt::CostShare s = adypt::cost_slot(node[adypt::kNodeMeta], adypt::cost_area(q, e), A);
	printf("%g %llu %llu %d %.3f\n", A, (unsigned long long)s.inner_q, (unsigned long long)s.leaf_q, (int)s.ok, adypt::cost_value(1.0, 0.5, s.inner_q, s.leaf_q));
	return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ to compile the driver with")
def test_header_needs_no_hip(tmp_path):
    (tmp_path / "driver.cpp").write_text(DRIVER)
    exe = str(tmp_path / "driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + DEVICE, str(tmp_path / "driver.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    assert out == ["24", "0", str(1 << 30), "1", "1.500"]
