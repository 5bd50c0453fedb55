"""-m gpu: every entry of the library that builds a tree takes the SAH costs, a method, a PLOC radius and a split budget, and checks them by
csrc/device/build_request.hpp (tests/test_build_request.py holds the header).  Here the entries themselves, through the C ABI: what each refuses, with
the text it has always given — the FIRST fault's when several arguments are wrong at once — and that a refusal changes nothing; that NULL costs are
0.3 / 1.0 to the byte; and that two shards pose and update under a policy as one device does.  Every refusal happens before the device is touched."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from tests import pose_truth as P  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_gpu_pose import gentle  # noqa: E402
from tests.test_gpu_refit import case_of, pose, tracer  # noqa: E402
from tests.test_refit_definition import same_bytes  # noqa: E402

NM = 4  # parts of the binding
NAN, INF = float("nan"), float("inf")
FLT_MAX = float(np.finfo(np.float32).max)

# the reasons as the entry points give them, behind "<entry>: "
SAH = "the SAH costs must be positive finite numbers"
METHOD = "method must be 0 (linear) or 1 (ploc)"
RADIUS = "the radius must be in [1, 32]"
BUDGET = "the split budget must be in [0, 1]"
NEEDS_PLOC = "a split budget needs method 1 (ploc)"
ABOVE = "rebuild_above must be a finite number >= 0"


def cfg(t=0.3, n=1.0):
    return N.BvhParams(0, t, n)


BAD = cfg(-1.0, 1.0)


def snapshot(p):
    return p.GetTriangleCount(), p.GetBVHSizes(), p.GetSPP(), p.ReadBVH()


def unchanged(p, before):
    now = snapshot(p)
    return now[:3] == before[:3] and same_bytes(now[3][0], before[3][0]) and np.array_equal(bits(now[3][1]), bits(before[3][1]))


def test_refusals_give_the_first_reason_and_change_nothing(scene_cache):
    case = case_of("tiny0", scene_cache)
    n = len(case.tris)
    p = tracer(case, case.scene, case.bvh(48))
    c, L = p._ctx, N.lib
    p.BindParts(P.parts_of(n, NM), NM)
    p.Trace(True, 2)
    before = snapshot(p)
    assert before[2] == 2
    tri = np.ascontiguousarray(case.scene.triangles).view(np.uint8).reshape(-1)
    pos = np.ascontiguousarray(pose(case.tris)["p"].reshape(-1, 9), dtype=np.float32)
    mats = np.ascontiguousarray(gentle(NM).reshape(-1, 12), dtype=np.float32)
    info, out, cost = N.RebuildInfo(), N.PoseOutcome(), N.TreeCost()

    def set_triangles(t, count, params, method, radius, budget):
        return L.adypt_set_triangles(c, t, count, params, method, radius, budget, C.byref(info))

    def update(positions, params, policy):
        return L.adypt_update_triangles_auto(c, 0, n, positions, None, params, None if policy is None else C.byref(N.PosePolicy(*policy)), C.byref(out))

    def posed(m, params, policy):
        return L.adypt_pose(c, m, NM, params, C.byref(N.PosePolicy(*policy)), C.byref(out))

    T, X, M = tri.ctypes.data, pos.ctypes.data, mats.ctypes.data
    refusals = [
        # ---- adypt_rebuild_bvh: the costs alone
        ("adypt_rebuild_bvh", SAH, lambda: L.adypt_rebuild_bvh(c, BAD, C.byref(info))),
        ("adypt_rebuild_bvh", SAH, lambda: L.adypt_rebuild_bvh(c, cfg(0.3, NAN), C.byref(info))),
        ("adypt_rebuild_bvh", SAH, lambda: L.adypt_rebuild_bvh(c, cfg(FLT_MAX, 1.0), C.byref(info))),
        ("adypt_rebuild_bvh", SAH, lambda: L.adypt_rebuild_bvh(c, cfg(0.3, 0.0), C.byref(info))),
        # ---- adypt_rebuild_bvh_ploc: the costs, then the radius
        ("adypt_rebuild_bvh_ploc", SAH, lambda: L.adypt_rebuild_bvh_ploc(c, BAD, 8, C.byref(info))),
        ("adypt_rebuild_bvh_ploc", RADIUS, lambda: L.adypt_rebuild_bvh_ploc(c, None, 0, C.byref(info))),
        ("adypt_rebuild_bvh_ploc", RADIUS, lambda: L.adypt_rebuild_bvh_ploc(c, cfg(), 33, C.byref(info))),
        ("adypt_rebuild_bvh_ploc", SAH, lambda: L.adypt_rebuild_bvh_ploc(c, BAD, 0, C.byref(info))),
        # ---- adypt_rebuild_bvh_ploc_split: the costs, the radius, then the budget's range
        ("adypt_rebuild_bvh_ploc_split", SAH, lambda: L.adypt_rebuild_bvh_ploc_split(c, cfg(INF, 1.0), 8, 0.25, C.byref(info))),
        ("adypt_rebuild_bvh_ploc_split", RADIUS, lambda: L.adypt_rebuild_bvh_ploc_split(c, None, -1, 0.25, C.byref(info))),
        ("adypt_rebuild_bvh_ploc_split", BUDGET, lambda: L.adypt_rebuild_bvh_ploc_split(c, None, 8, 1.5, C.byref(info))),
        ("adypt_rebuild_bvh_ploc_split", BUDGET, lambda: L.adypt_rebuild_bvh_ploc_split(c, None, 8, NAN, C.byref(info))),
        ("adypt_rebuild_bvh_ploc_split", BUDGET, lambda: L.adypt_rebuild_bvh_ploc_split(c, None, 8, -1e-9, C.byref(info))),
        ("adypt_rebuild_bvh_ploc_split", SAH, lambda: L.adypt_rebuild_bvh_ploc_split(c, BAD, 33, NAN, C.byref(info))),
        ("adypt_rebuild_bvh_ploc_split", RADIUS, lambda: L.adypt_rebuild_bvh_ploc_split(c, None, 33, NAN, C.byref(info))),
        # ---- adypt_set_triangles: its own two, the costs, then method, radius, range, needs-ploc
        ("adypt_set_triangles", "triangles is null", lambda: set_triangles(None, n, None, 1, 8, 0.0)),
        ("adypt_set_triangles", "the number of triangles must be in [1, 2^30]", lambda: set_triangles(T, 0, None, 1, 8, 0.0)),
        ("adypt_set_triangles", SAH, lambda: set_triangles(T, n, BAD, 1, 8, 0.0)),
        ("adypt_set_triangles", METHOD, lambda: set_triangles(T, n, None, 2, 8, 0.0)),
        ("adypt_set_triangles", METHOD, lambda: set_triangles(T, n, None, -1, 8, 0.0)),
        ("adypt_set_triangles", RADIUS, lambda: set_triangles(T, n, None, 1, 0, 0.0)),
        ("adypt_set_triangles", BUDGET, lambda: set_triangles(T, n, None, 1, 8, -0.1)),
        ("adypt_set_triangles", NEEDS_PLOC, lambda: set_triangles(T, n, None, 0, 8, 0.25)),
        ("adypt_set_triangles", "triangles is null", lambda: set_triangles(None, 0, BAD, 2, 0, NAN)),
        ("adypt_set_triangles", "the number of triangles must be in [1, 2^30]", lambda: set_triangles(T, 0, BAD, 1, 8, 0.0)),
        ("adypt_set_triangles", SAH, lambda: set_triangles(T, n, BAD, 2, 8, 0.0)),
        ("adypt_set_triangles", METHOD, lambda: set_triangles(T, n, None, 2, 99, NAN)),
        ("adypt_set_triangles", RADIUS, lambda: set_triangles(T, n, None, 1, 0, 2.0)),
        ("adypt_set_triangles", BUDGET, lambda: set_triangles(T, n, None, 0, 0, 1.5)),  # (out of range before "needs ploc")
        # ---- adypt_update_triangles_auto: its own, the costs, rebuild_above, then method, radius, range, needs-ploc
        ("adypt_update_triangles_auto", "positions is null", lambda: update(None, BAD, (1.0, 1, 8, 0.0))),
        ("adypt_update_triangles_auto", "policy is null", lambda: update(X, BAD, None)),
        ("adypt_update_triangles_auto", SAH, lambda: update(X, BAD, (1.0, 1, 8, 0.0))),
        ("adypt_update_triangles_auto", ABOVE, lambda: update(X, None, (NAN, 1, 8, 0.0))),
        ("adypt_update_triangles_auto", ABOVE, lambda: update(X, None, (-1.0, 1, 8, 0.0))),
        ("adypt_update_triangles_auto", ABOVE, lambda: update(X, None, (INF, 1, 8, 0.0))),
        ("adypt_update_triangles_auto", METHOD, lambda: update(X, None, (1.0, 2, 8, 0.0))),
        ("adypt_update_triangles_auto", RADIUS, lambda: update(X, None, (1.0, 1, 33, 0.0))),
        ("adypt_update_triangles_auto", BUDGET, lambda: update(X, None, (1.0, 1, 8, 1.5))),
        ("adypt_update_triangles_auto", NEEDS_PLOC, lambda: update(X, None, (1.0, 0, 8, 0.5))),
        ("adypt_update_triangles_auto", SAH, lambda: update(X, BAD, (NAN, 2, 0, NAN))),
        ("adypt_update_triangles_auto", ABOVE, lambda: update(X, None, (NAN, 2, 8, 0.0))),  # (rebuild_above stands between the costs and the method)
        ("adypt_update_triangles_auto", METHOD, lambda: update(X, None, (0.0, 2, 0, 1.5))),
        # ---- adypt_pose with a policy: the same
        ("adypt_pose", "matrices is null", lambda: posed(None, BAD, (NAN, 2, 8, 0.0))),
        ("adypt_pose", SAH, lambda: posed(M, BAD, (1.0, 1, 8, 0.0))),
        ("adypt_pose", ABOVE, lambda: posed(M, None, (NAN, 1, 8, 0.0))),
        ("adypt_pose", METHOD, lambda: posed(M, None, (1.0, 2, 8, 0.0))),
        ("adypt_pose", RADIUS, lambda: posed(M, None, (1.0, 1, 0, 0.0))),
        ("adypt_pose", BUDGET, lambda: posed(M, None, (1.0, 1, 8, NAN))),
        ("adypt_pose", NEEDS_PLOC, lambda: posed(M, None, (1.0, 0, 8, 1.0))),
        ("adypt_pose", SAH, lambda: posed(M, cfg(0.3, -0.0), (-1.0, 1, 0, 0.0))),
        ("adypt_pose", ABOVE, lambda: posed(M, None, (NAN, 2, 8, 0.0))),
        ("adypt_pose", RADIUS, lambda: posed(M, None, (0.0, 1, 33, 7.0))),
        # ---- adypt_get_tree_cost: the costs alone
        ("adypt_get_tree_cost", SAH, lambda: L.adypt_get_tree_cost(c, BAD, C.byref(cost))),
        ("adypt_get_tree_cost", SAH, lambda: L.adypt_get_tree_cost(c, cfg(NAN, NAN), C.byref(cost))),
        ("adypt_get_tree_cost", "out is null", lambda: L.adypt_get_tree_cost(c, BAD, None)),
    ]
    for i, (who, why, call) in enumerate(refusals):
        assert call() == N.E_INVALID, (i, who, why)
        assert L.adypt_last_error(c).decode() == who + ": " + why, i
        assert unchanged(p, before), (i, who, why)
    assert p.GetPoseBinding()["kind"] == 1
    # what is no fault: a radius out of range with the linear method, and a budget of -0.0
    assert set_triangles(T, n, None, 0, 99, -0.0) == N.ADYPT_OK and L.adypt_rebuild_bvh_ploc_split(c, None, 1, -0.0, C.byref(info)) == N.ADYPT_OK
    p.destroy()


def test_null_costs_are_the_defaults_to_the_byte(scene_cache):
    case = case_of("tiny0", scene_cache)
    n = len(case.tris)
    parts, mats, moved = P.parts_of(n, NM), gentle(NM), pose(case.tris)
    pos = moved["p"].reshape(-1, 9)
    a, b = (tracer(case, case.scene, case.bvh(48)) for _ in range(2))

    def same_tree(what):
        (na, wa), (nb, wb) = a.ReadBVH(), b.ReadBVH()
        assert a.GetBVHSizes() == b.GetBVHSizes() and same_bytes(na, nb) and np.array_equal(bits(wa), bits(wb)), what
        assert np.array_equal(a.ReadTriIndices(), b.ReadTriIndices()), what

    entries = [
        ("adypt_rebuild_bvh", lambda p, c: p.RebuildBVH(c)),
        ("adypt_rebuild_bvh_ploc", lambda p, c: p.RebuildBVH(c, method="ploc", radius=4)),
        ("adypt_rebuild_bvh_ploc_split", lambda p, c: p.RebuildBVH(c, method="ploc", split_budget=0.3)),
        ("adypt_set_triangles", lambda p, c: p.SetTriangles(moved, c, method="ploc")),
        ("adypt_update_triangles_auto", lambda p, c: p.UpdateTriangles(0, pos, rebuild_above=0.0, method="linear", cfg=c)),
        ("adypt_pose", lambda p, c: (p.BindParts(parts, NM), p.Pose(mats, rebuild_above=0.0, cfg=c))[1]),
        ("adypt_get_tree_cost", lambda p, c: p.GetTreeCost(c)),
    ]
    for who, call in entries:
        ra, rb = call(a, None), call(b, cfg())
        if "rebuilt" in ra:
            assert ra["rebuilt"] == rb["rebuilt"] == 1, who
            ra, rb = dict(ra, cost_ms=0.0), dict(rb, cost_ms=0.0)
        assert ra == rb, who
        same_tree(who)
    # ... and other costs are looked at: with a triangle at 40 times the price of a node slot the collapse cuts leaves apart that the defaults keep
    a.RebuildBVH(None, method="ploc")
    b.RebuildBVH(cfg(4.0, 0.1), method="ploc")
    assert a.GetTreeCost() != b.GetTreeCost()
    for p in (a, b):
        p.destroy()


def test_two_shards_decide_as_one_device(scene_cache, monkeypatch):
    """adypt_multi_pose and adypt_multi_update_triangles_auto hold every device's outcome against the first one's: the success path of that check"""
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = case_of("tiny0", scene_cache)
    n = len(case.tris)
    parts, mats = P.parts_of(n, NM), np.ascontiguousarray(gentle(NM).reshape(-1, 12), dtype=np.float32)
    pos = np.ascontiguousarray(pose(case.tris)["p"].reshape(-1, 9), dtype=np.float32)
    w, h = 64, 36  # 2 x 2 blocks: both shards own some
    single = tracer(case, case.scene, case.bvh(48), w, h)
    multi = tracer(case, case.scene, case.bvh(48), w, h, cls=api.MultiPathTracer, devices=(0, 0))
    assert multi.DeviceCount() == 2
    policies = [(1e9, 1, 8, 0.0), (0.0, 1, 8, 0.0), (0.0, 0, 8, 0.0), (0.0, 1, 4, 0.3)]
    outcomes = {}
    for name, t in (("single", single), ("multi", multi)):
        t.BindParts(parts, NM)
        family = "adypt_multi_" if t is multi else "adypt_"
        got = []
        for policy in policies:
            for call in ("pose", "update_triangles_auto"):
                out, pol = N.PoseOutcome(), N.PosePolicy(*policy)
                args = (mats.ctypes.data, NM) if call == "pose" else (0, n, pos.ctypes.data, None)
                code = getattr(N.lib, family + call)(t._h, *args, None, C.byref(pol), C.byref(out))
                assert code == N.ADYPT_OK, (name, call, policy, N.lib.adypt_multi_last_error(t._h) if t is multi else N.lib.adypt_last_error(t._h))
                got.append(dict(out.as_dict(), cost_ms=0.0))
        outcomes[name] = got
    assert outcomes["multi"] == outcomes["single"]
    assert [o["rebuilt"] for o in outcomes["single"]] == [0, 0, 1, 1, 1, 1, 1, 1]
    want = single.ReadBVH()
    for c in multi._contexts():  # every device holds the tree the one device holds
        nodes, woop = np.zeros_like(want[0]), np.zeros_like(want[1])
        N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, woop.ctypes.data), c)
        assert same_bytes(nodes, want[0]) and np.array_equal(bits(woop), bits(want[1]))
    multi.destroy()
    single.destroy()
