"""-m gpu: the SAH cost of the tree on the device (include/adypt_hip.h adypt_get_tree_cost; k_tree_cost in csrc/device/refit.hip, the definition
csrc/device/tree_cost.hpp) and the refit that rebuilds when the cost says so (adypt_update_triangles_auto).  The device's two integers are held against
the host's adypt_bvh_cost (and that against numpy in tests/test_tree_cost_definition.py); what the policy call leaves behind — nodes, Woop data,
reference order, image — against a twin context that made the plain calls, bit for bit; its decisions against a host simulation with
WideBVH.Refit / BuildPLOC / Cost, exactly.  A workgroup of k_tree_cost takes 32 nodes, a wave 8: the trees have 1 node, 3 nodes, counts above 32
that are no multiple of 8 or of 32, and 456 nodes (15 workgroups)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from tests import refit_truth as RT  # noqa: E402
from tests import tree_cost_truth as T  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_gpu_rebuild import Loose  # noqa: E402
from tests.test_gpu_refit import case_of, same_woop, tracer, update  # noqa: E402
from tests.test_refit_definition import same_bytes  # noqa: E402

W, H, SPP = 64, 48, 2
ABOVE = 1.4
_ploc = {}


def cfg():
    return api.InstanceConfig().bvh_params()


def host_cost(nodes):
    b = api.WideBVH()
    b.nodes = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    return b.Cost()


def ploc_of(tris, mats):
    b = api.WideBVH()
    b.BuildPLOC(api.Scene.FromArrays(tris, mats), cfg())
    return b


def refitted(b, tris, mats):
    c = api.WideBVH()
    c.nodes, c.tri_indices = np.array(b.nodes), np.array(b.tri_indices)
    c.Refit(api.Scene.FromArrays(tris, mats))
    return c


def rest_ploc(case):
    """WideBVH.BuildPLOC of the soup's rest pose; shared and never written"""
    if "rest" not in _ploc:
        _ploc["rest"] = ploc_of(case.tris, case.scene.materials)
        _ploc["rest"].nodes.setflags(write=False)
    return _ploc["rest"]


def costs(outcome):
    """an outcome without its timing"""
    return {k: outcome[k] for k in ("built", "refitted", "now", "rebuilt")}


def state(p):
    nodes, woop = p.ReadBVH()
    return nodes, woop, p.ReadTriIndices()


def same_state(a, b):
    return same_bytes(a[0], b[0]) and same_woop(a[1], b[1]) and np.array_equal(a[2], b[2])


def image(p):
    p.Trace(True, SPP)
    return p.ReadResult()


def linear_soup(pred):
    """a soup whose linear tree has a node count with the property asked for"""
    for n in range(600, 700):
        case = Loose(RT.soup(n, 21))
        b = api.WideBVH()
        b.BuildLinear(case.scene, cfg())
        if pred(len(b.nodes) // 80):
            return case, b
    raise AssertionError("no soup of 600 .. 699 triangles has such a tree")


def small(n):
    case = Loose(RT.soup(n, 3))
    b = api.WideBVH()
    b.Build(case.scene, cfg())
    return case, b


SHAPES = {
    "tiny0": lambda cache: (case_of("tiny0", cache), case_of("tiny0", cache).bvh(48)),
    "soup": lambda cache: (case_of("soup", cache), case_of("soup", cache).bvh(48)),
    "one_triangle": lambda cache: small(1),
    "nine_triangles": lambda cache: small(9),
    "thirty_triangles": lambda cache: small(30),
    "ragged_wave": lambda cache: linear_soup(lambda k: k > 32 and k % 8 != 0),
    "ragged_group": lambda cache: linear_soup(lambda k: k > 32 and k % 8 == 0 and k % 32 != 0),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_device_equals_host(shape, scene_cache):
    case, b = SHAPES[shape](scene_cache)
    n_nodes = len(b.nodes) // 80
    assert shape != "one_triangle" or n_nodes == 1
    assert shape != "thirty_triangles" or 1 < n_nodes < 8
    p = tracer(case, case.scene, b)
    before = state(p)
    got, want = p.GetTreeCost(), b.Cost()
    print(shape, n_nodes, "nodes:", got)
    assert got == want and got["n_nodes"] == n_nodes and got["leaf_q"] > 0
    assert p.GetTreeCost() == want                      # (the sums start from zero every time)
    other = cfg()
    other.triangle_sah, other.node_sah = 0.7, 2.5
    assert p.GetTreeCost(other) == b.Cost(other)
    assert same_state(state(p), before)
    p.destroy()


def test_after_every_change_of_tree(scene_cache):
    case = case_of("soup", scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    update(p, RT.wave(case.tris))
    assert p.GetTreeCost() == host_cost(p.ReadBVH()[0])
    sizes = set()
    for kw in (dict(method="linear"), dict(method="ploc"), dict(method="ploc", split_budget=0.3)):
        p.RebuildBVH(**kw)
        got = p.GetTreeCost()
        assert got == host_cost(p.ReadBVH()[0]) and got["n_nodes"] == p.GetBVHSizes()[0]
        sizes.add((got["inner_q"], got["leaf_q"]))
    assert len(sizes) == 3
    p.destroy()


def test_kept(scene_cache):
    case = case_of("soup", scene_cache)
    b = rest_ploc(case)
    moved = T.apart(case.tris, 0.05)
    p, twin = (tracer(case, case.scene, case.bvh(48), W, H) for _ in range(2))
    for t in (p, twin):
        t.RebuildBVH(method="ploc")
        t.Trace(True, 1)
    out = p.UpdateTriangles(0, moved["p"].reshape(-1, 9), rebuild_above=ABOVE)
    update(twin, moved)
    kept = refitted(b, moved, case.scene.materials)
    assert out["rebuilt"] == 0 and p.GetSPP() == 0
    assert costs(out) == {"built": b.Cost(), "refitted": kept.Cost(), "now": kept.Cost(), "rebuilt": 0}
    assert out["refitted"]["cost"] <= ABOVE * out["built"]["cost"] and out["cost_ms"] > 0.0
    assert all(v == 0 for v in out["rebuild"].values())
    assert same_state(state(p), state(twin)) and same_bytes(p.ReadBVH()[0], kept.nodes)
    a = image(p)
    assert np.array_equal(bits(a), bits(image(twin))) and a.any()
    p.destroy()
    twin.destroy()


def test_rebuilt(scene_cache):
    case = case_of("soup", scene_cache)
    mats = case.scene.materials
    b = rest_ploc(case)
    moved = T.apart(case.tris, 1.5)
    p, twin = (tracer(case, case.scene, case.bvh(48), W, H) for _ in range(2))
    for t in (p, twin):
        t.RebuildBVH(method="ploc")
        t.Trace(True, 1)
    out = p.UpdateTriangles(0, moved["p"].reshape(-1, 9), rebuild_above=ABOVE)
    update(twin, moved)
    info = twin.RebuildBVH(method="ploc")
    fresh = ploc_of(moved, mats)
    assert out["rebuilt"] == 1 and p.GetSPP() == 0
    assert costs(out) == {"built": b.Cost(), "refitted": refitted(b, moved, mats).Cost(), "now": fresh.Cost(), "rebuilt": 1}
    assert out["refitted"]["cost"] > ABOVE * out["built"]["cost"]
    assert out["rebuild"] == info and same_state(state(p), state(twin)) and same_bytes(p.ReadBVH()[0], fresh.nodes)
    assert p.GetTreeCost() == out["now"]
    # the reference moved to the new tree: a small step from there is kept
    step = T.apart(case.tris, 1.55)
    out = p.UpdateTriangles(0, step["p"].reshape(-1, 9), rebuild_above=ABOVE)
    update(twin, step)
    kept = refitted(fresh, step, mats)
    assert costs(out) == {"built": fresh.Cost(), "refitted": kept.Cost(), "now": kept.Cost(), "rebuilt": 0}
    assert same_state(state(p), state(twin))
    a = image(p)
    assert np.array_equal(bits(a), bits(image(twin))) and a.any()
    p.destroy()
    twin.destroy()


def test_a_walk(scene_cache):
    case = case_of("soup", scene_cache)
    mats = case.scene.materials
    p = tracer(case, case.scene, case.bvh(48))
    p.RebuildBVH(method="ploc")
    b = rest_ploc(case)
    built = b.Cost()
    flags = []
    for k in range(11):
        moved = T.apart(case.tris, 0.05 * k)
        out = p.UpdateTriangles(0, moved["p"].reshape(-1, 9), rebuild_above=ABOVE)
        r = refitted(b, moved, mats)
        want = {"built": built, "refitted": r.Cost(), "now": r.Cost(), "rebuilt": 0}
        b = r
        if want["refitted"]["cost"] > ABOVE * built["cost"]:
            b = ploc_of(moved, mats)
            built = b.Cost()
            want.update(now=built, rebuilt=1)
        assert costs(out) == want, "step %d" % k
        flags.append(out["rebuilt"])
    print("rebuilt at steps", [k for k, f in enumerate(flags) if f])
    assert flags[0] == 0 and sum(flags) >= 1
    assert same_bytes(p.ReadBVH()[0], b.nodes) and np.array_equal(p.ReadTriIndices(), b.tri_indices)
    p.destroy()


def test_a_tree_with_spatial_splits_is_rebuilt_in_its_rest_pose(scene_cache):
    case = case_of("tiny1", scene_cache)
    b = case.bvh(48)
    assert len(b.tri_indices) > len(case.tris)
    p = tracer(case, case.scene, b)
    out = p.UpdateTriangles(0, case.tris["p"].reshape(-1, 9), rebuild_above=ABOVE)
    kept = refitted(b, case.tris, case.scene.materials)
    assert out["rebuilt"] == 1 and out["built"] == b.Cost() and out["refitted"] == kept.Cost()
    ratio = out["refitted"]["cost"] / out["built"]["cost"]
    print("tiny1, depth 48, refitted at rest: ratio %.3f" % ratio)
    assert abs(ratio - 10.46) < 0.01
    fresh = ploc_of(case.tris, case.scene.materials)
    assert out["now"] == fresh.Cost() and same_bytes(p.ReadBVH()[0], fresh.nodes)
    p.destroy()


def test_refusals_change_nothing(scene_cache):
    case = case_of("tiny0", scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    p.Trace(True, SPP)
    before, img = state(p), p.ReadResult()
    pos = np.ascontiguousarray(RT.wave(case.tris)["p"].reshape(-1, 9))
    n = len(pos)

    def refused(first, count, above, method=1, radius=8, budget=0.0, params=None):
        policy, out = N.PosePolicy(above, method, radius, budget), N.PoseOutcome()
        r = N.lib.adypt_update_triangles_auto(p._h, first, count, pos.ctypes.data, None, None if params is None else N.C.byref(params), N.C.byref(policy), N.C.byref(out))
        assert r == N.E_INVALID and N.lib.adypt_last_error(p._h)
        assert p.GetSPP() == SPP and same_state(state(p), before)

    for above in (float("nan"), -0.5, float("inf")):
        refused(0, n, above)
    refused(0, n, ABOVE, method=2)
    refused(0, n, ABOVE, radius=0)
    refused(0, n, ABOVE, budget=1.5)
    refused(0, n, ABOVE, method=0, budget=0.3)
    refused(n - 1, 2, ABOVE)
    refused(-1, 1, ABOVE)
    bad = cfg()
    bad.node_sah = float("nan")
    refused(0, n, ABOVE, params=bad)
    for kw in (dict(method="sah"), dict(method="linear", split_budget=0.3)):
        with pytest.raises(ValueError):
            p.UpdateTriangles(0, pos, rebuild_above=ABOVE, **kw)
    with pytest.raises(N.AdyptError) as e:
        p.GetTreeCost(bad)
    assert e.value.code == N.E_INVALID
    assert p.GetSPP() == SPP and same_state(state(p), before) and np.array_equal(bits(p.ReadResult()), bits(img))
    assert p.UpdateTriangles(0, pos) is None  # (the plain call is what it was)
    # a root without area after the refit: the cost cannot be taken, the refit stays
    point = np.full_like(pos, 1.25)
    with pytest.raises(N.AdyptError) as e:
        p.UpdateTriangles(0, point, rebuild_above=ABOVE)
    assert e.value.code == N.E_INVALID and "refitted" in str(e.value)
    q = tracer(case, case.scene, case.bvh(48))
    q.UpdateTriangles(0, point)
    assert same_bytes(p.ReadBVH()[0], q.ReadBVH()[0])
    q.destroy()
    p.destroy()


def test_two_shards_on_one_device(scene_cache, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = case_of("soup", scene_cache)
    single = tracer(case, case.scene, case.bvh(48), W, H)
    multi = tracer(case, case.scene, case.bvh(48), W, H, cls=api.MultiPathTracer, devices=(0, 0))
    assert multi.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in multi._contexts())
    for t in (single, multi):
        t.RebuildBVH(method="ploc")
    assert multi.GetTreeCost() == single.GetTreeCost()
    flags = []
    for f in (0.05, 1.5):
        moved = T.apart(case.tris, f)
        a, b = (t.UpdateTriangles(0, moved["p"].reshape(-1, 9), rebuild_above=ABOVE) for t in (single, multi))
        assert costs(a) == costs(b) and a["rebuild"] == b["rebuild"]
        flags.append(a["rebuilt"])
        want = state(single)
        for c in multi._contexts():
            nodes, woop, idx = np.zeros_like(want[0]), np.zeros_like(want[1]), np.zeros_like(want[2])
            N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, woop.ctypes.data), c)
            N.check(N.lib.adypt_read_tri_indices(c, idx.ctypes.data), c)
            assert same_state((nodes, woop, idx), want)
        assert np.array_equal(bits(image(multi)), bits(image(single)))
    assert flags == [0, 1]
    multi.destroy()
    single.destroy()
