"""-m gpu: adypt_trace_by_history — the plan followed by the tracing (include/adypt_hip.h; csrc/device/history_reach.hpp trace_plan, history_plan.hip).
The plan is held against the truth's (tests/history_reach_truth.py, from the CPU ORACLE's guides and the truth's own history), the radiance block by
block against the oracle's uniform image at each block's count (the method of tests/test_gpu_adaptive.py), the merge's history length against
block count + reach.  Also here: a plan alone changes no bit of what follows, the refusals, and several shards on one card.  tiny0 100x75."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from tests import history_reach_truth as HT  # noqa: E402
from tests import temporal_truth as TT  # noqa: E402
from tests import test_gpu_denoise as DN  # noqa: E402
from tests import test_gpu_denoise_temporal as TG  # noqa: E402
from tests import test_gpu_noise as G  # noqa: E402
from tests.helpers import bits, oracle_scene_from_instance  # noqa: E402

CASE = G.CASES[0]
NAME, W, H = CASE[:3]
SPP = TG.SPP
F = np.float32
PLAN = dict(target=12, min_spp=2, max_spp=16, step=4)
FRAMES = 10  # the largest count the truth plans at the third pose
same = TG.same


def poses_of(inst, sobol_matrices):
    """TG's three poses, and the oracle's image after every frame up to FRAMES at the third"""
    poses = TG.sequence(inst, CASE, sobol_matrices)
    c = inst.m_config.c
    pos, yaw = TG.camera_of(c, NAME, 2)
    _, _, images, _ = TG.oracle_pose(CASE[:5] + (2, "by history"), oracle_scene_from_instance(inst), c, pos, yaw, TG.SEED + 2, sobol_matrices, frames=FRAMES)
    return poses, images


def commit_two(t, cfg, poses):
    """the first two poses traced at SPP and committed; the truth's history"""
    hist = None
    for k in (0, 1):
        pos, yaw, seed, call, cam = poses[k][:5]
        TG.set_pose(t, cfg, pos, yaw, seed)
        t.Denoise(temporal=True)
        _, _, hist = TT.denoise(*call, hist, cam)
    return hist


def truth_plan(call, hist, **kw):
    A, Nn, P, hit = call[3:7]
    reach = HT.reach(Nn, P, A, hit, hist)
    args = dict(PLAN, **kw)
    return reach, HT.plan(HT.bins(reach, hit), args["target"], args["min_spp"], args["max_spp"], args["step"], args.get("tolerance_permille", 31))


def assert_blocks_are_the_oracles(got, images, want, tag):
    for b, ys, xs in HT.blocks_of(W, H):
        assert same(got[ys, xs], images[want[b] - 1][ys, xs]), "%s: block %d is not the oracle's image after %d frames" % (tag, b, want[b])


def test_the_plan_is_traced_and_the_merge_finds_what_it_foresaw(scene_cache, sobol_matrices):
    inst, _ = G._instance(scene_cache, CASE)
    p, cfg = inst.m_path_tracer, inst.m_config
    p.SetNoiseStats(True)
    poses, images = poses_of(inst, sobol_matrices)
    hist = commit_two(p, cfg, poses)
    pos, yaw, seed, call, cam = poses[2][:5]
    reach, want = truth_plan(call, hist)
    assert sorted(set(want)) == [2, 6, FRAMES], "the case: three groups, two of them frozen (%s)" % want
    TG.set_pose(p, cfg, pos, yaw, seed, 0)
    info = p.TraceByHistory(**PLAN)
    idx, plan = p.ReadSamplePlan()
    assert np.array_equal(idx, np.arange(12)) and np.array_equal(plan, want), "the plan %s, the truth's %s" % (plan, want)
    assert np.array_equal(p.ReadBlockSPP()[1], want) and p.GetSPP() == FRAMES == info["spp"] == info["want_max"] and info["want_min"] == 2
    assert info["pixel_samples"] == HT.pixel_samples(want, W, H) < PLAN["target"] * W * H and info["pixels"] == W * H
    assert same(p.ReadHistoryReach(), reach)
    assert_blocks_are_the_oracles(p.ReadResult(), images, want, "after TraceByHistory")
    p.Denoise(temporal=True, commit=False)
    n = HT.per_pixel(want, W, H).astype(np.float32)
    assert same(p.ReadDenoiseHistory(), np.where(reach > 0, n + reach, n).astype(np.float32)), "the merge found another length than block count + reach"
    # the blocks of the largest count are still active: tracing on moves them alone
    p.Trace(True, 0)
    assert np.array_equal(p.ReadBlockSPP()[1], want)
    # a refusal now (frames traced, blocks frozen) leaves everything, and after a reset the same call gives the same image
    before = DN.state_of(p)
    for call_ in (p.PlanByHistory, p.TraceByHistory):
        with pytest.raises(N.AdyptError) as e:
            call_(**PLAN)
        assert e.value.code == N.E_STATE and "blocks are frozen" in str(e.value), str(e.value)
    DN.assert_same_state(DN.state_of(p), before, "around the refused calls")
    assert np.array_equal(p.ReadSamplePlan()[1], want), "a refused call dropped the last plan"
    TG.set_pose(p, cfg, pos, yaw, seed, 0)
    p.TraceByHistory(**PLAN)
    assert np.array_equal(p.ReadBlockSPP()[1], want)
    assert_blocks_are_the_oracles(p.ReadResult(), images, want, "the second time")
    # a single distinct count: one trace, nothing frozen
    TG.set_pose(p, cfg, pos, yaw, seed, 0)
    info = p.TraceByHistory(target=1, min_spp=6, max_spp=16, step=4)
    assert info["want_min"] == info["want_max"] == 6 == p.GetSPP() and (p.ReadBlockSPP()[1] == 6).all()
    assert same(p.ReadResult(), images[5])
    p.destroy()


def test_a_plan_alone_changes_no_bit_of_what_follows(scene_cache, sobol_matrices):
    inst, _ = G._instance(scene_cache, CASE)
    p, cfg = inst.m_path_tracer, inst.m_config
    p.SetNoiseStats(True)
    poses = TG.sequence(inst, CASE, sobol_matrices)
    out = []
    for with_plan in (True, False):
        p.ResetDenoiseHistory()
        hist = commit_two(p, cfg, poses)
        pos, yaw, seed, call, cam = poses[2][:5]
        TG.set_pose(p, cfg, pos, yaw, seed, 0)
        if with_plan:
            p.PlanByHistory(**PLAN)
            p.PlanByHistory(moments=True, follow_motion=True, **PLAN)
        p.Trace(True, SPP)
        assert same(p.ReadResult(), call[0]), "the image is not the oracle's"
        want, want_n, new = TT.denoise(*call, hist, cam)
        got = p.Denoise(temporal=True)
        assert same(got, want) and same(p.ReadDenoiseHistory(), want_n), "with the plan: %s" % with_plan
        # the next pose (back under the first camera) finds the history this one committed
        pos, yaw, seed, call, cam = poses[0][:5]
        TG.set_pose(p, cfg, pos, yaw, seed)
        nxt, nxt_n = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
        want, want_n, _ = TT.denoise(*call, new, cam)
        assert same(nxt, want) and same(nxt_n, want_n), "the next pose, with the plan: %s" % with_plan
        out.append((got, nxt, nxt_n))
    assert all(same(a, b) for a, b in zip(*out))
    p.destroy()


def test_refusals(scene_cache, sobol_matrices):
    inst, _ = G._instance(scene_cache, CASE)
    p, cfg = inst.m_path_tracer, inst.m_config
    poses = TG.sequence(inst, CASE, sobol_matrices)
    pos, yaw, seed, call, cam = poses[0][:5]
    _, want = truth_plan(call, None)

    def refused(code, word, **kw):
        before = (p.GetSPP(), p.ReadBlockSPP()[1].copy(), p.ReadResult(), p.GetLookaheadFrames())
        for fn in (p.PlanByHistory, p.TraceByHistory):
            with pytest.raises(N.AdyptError) as e:
                fn(**dict(PLAN, **kw))
            assert e.value.code == code and word in str(e.value), (kw, str(e.value))
        after = (p.GetSPP(), p.ReadBlockSPP()[1], p.ReadResult(), p.GetLookaheadFrames())
        assert before[0] == after[0] and np.array_equal(before[1], after[1]) and same(before[2], after[2]) and before[3] == after[3], "a refused call changed something"

    def works():
        TG.set_pose(p, cfg, pos, yaw, seed, 0)
        p.TraceByHistory(**PLAN)
        assert np.array_equal(p.ReadBlockSPP()[1], want) and np.array_equal(p.ReadSamplePlan()[1], want)
        TG.set_pose(p, cfg, pos, yaw, seed, 0)

    TG.set_pose(p, cfg, pos, yaw, seed, 0)
    refused(N.E_STATE, "statistics")                    # the statistics are off
    p.SetNoiseStats(True)
    works()
    p.SetLookahead(True)
    refused(N.E_STATE, "look-ahead")
    p.SetLookahead(False)
    works()
    p.Trace(True, 2)
    refused(N.E_STATE, "before the first sample")       # spp > 0
    works()
    p.TraceAdaptive(1e9, 2, 4, 2)                       # every block freezes at 2 spp
    assert (p.ReadBlockSPP()[1] == 2).all()
    refused(N.E_STATE, "blocks are frozen")
    works()
    for kw in (dict(target=0), dict(target=(1 << 20) + 1), dict(min_spp=1), dict(min_spp=17), dict(step=0), dict(tolerance_permille=-1), dict(tolerance_permille=1000),
               dict(history_cap=0.0), dict(history_cap=float("nan")), dict(history_cap=float("inf"))):
        refused(N.E_INVALID, "needs 1 <= target", **kw)
    works()
    # null parameters: the defaults (target 16, 2, 64, 4, 31, 64.0)
    assert N.lib.adypt_plan_by_history(p._ctx, None, None) == N.ADYPT_OK
    assert np.array_equal(p.ReadSamplePlan()[1], truth_plan(call, None, target=16, max_spp=64)[1])
    p.destroy()
    # a context without a camera
    bare = api.HipPathTracer()
    bare.Initialize(cfg.pt_params(seed), inst.m_hipscene, W, H)
    bare.SetNoiseStats(True)
    with pytest.raises(N.AdyptError) as e:
        bare.PlanByHistory(**PLAN)
    assert e.value.code == N.E_STATE and "adypt_set_camera" in str(e.value)
    bare.destroy()
    # a shard context
    part = TG.make_instance(scene_cache, "tiny0", W, H, rank=1, world=2)
    q = part.m_path_tracer
    q.SetNoiseStats(True)
    for fn in (q.PlanByHistory, q.TraceByHistory):
        with pytest.raises(N.AdyptError) as e:
            fn(**PLAN)
        assert e.value.code == N.E_STATE and "tile shard" in str(e.value)
    assert q.GetSPP() == 0
    q.destroy()


@pytest.mark.parametrize("n_dev", [2, 3])
def test_multi_device_on_one_card(n_dev, scene_cache, sobol_matrices, monkeypatch):
    """Several shards on one card against one context: the same plan, the same reach and bins, the same image, the same merge."""
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    inst, _ = G._instance(scene_cache, CASE)
    single, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    single.SetNoiseStats(True)
    m = api.MultiPathTracer()
    m.Initialize(cfg.pt_params(TG.SEED), inst.m_hipscene, c.width, c.height, (0,) * n_dev)
    assert m.DeviceCount() == n_dev
    m.SetNoiseStats(True)
    poses = TG.sequence(inst, CASE, sobol_matrices)
    pos, yaw, seed, call, cam = poses[2][:5]
    out = []
    for t in (single, m):
        hist = commit_two(t, cfg, poses)
        TG.set_pose(t, cfg, pos, yaw, seed, 0)
        plan_info = t.PlanByHistory(**PLAN)
        plan_only = (t.ReadSamplePlan(), t.GetSPP(), t.ReadBlockSPP()[1].copy())
        info = t.TraceByHistory(**PLAN)
        den = t.Denoise(temporal=True, commit=False)
        out.append(dict(plan=t.ReadSamplePlan(), reach=t.ReadHistoryReach(), bins=t.ReadHistoryBins(), spp=t.ReadBlockSPP(), image=t.ReadResult(), den=den, length=t.ReadDenoiseHistory(),
                        info=info, plan_info=plan_info, plan_only=plan_only))
    a, b = out
    reach, want = truth_plan(call, hist)
    assert np.array_equal(a["plan"][1], want) and same(a["reach"], reach), "one context against the truth"
    for key in ("plan", "bins", "spp"):
        assert all(np.array_equal(x, y) for x, y in zip(a[key], b[key])), "%d shards against one context: %s" % (n_dev, key)
    for key in ("reach", "image", "den", "length"):
        assert same(a[key], b[key]), "%d shards against one context: %s" % (n_dev, key)
    for key in ("blocks", "want_min", "want_max", "spp", "pixels", "pixels_with_history", "pixel_samples", "mean_reach"):
        assert a["info"][key] == b["info"][key] and a["plan_info"][key] == b["plan_info"][key], key
    assert b["plan_only"][1] == 0 and (b["plan_only"][2] == 0).all() and np.array_equal(b["plan_only"][0][1], want), "the plan of several devices traced or froze something"
    m.destroy()
    single.destroy()
