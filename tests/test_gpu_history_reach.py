"""-m gpu: the reach kernel of history-aware sampling (include/adypt_hip.h adypt_plan_by_history ...; csrc/device/history_reach.hpp, k_history_reach
in history_plan.hip).  The truth is computed in this process by the numpy restatement (tests/history_reach_truth.py) from what the CPU ORACLE gives
for every pose — its primary frames of types 0 / 4 / 5, the triangle and (u, v) of its primary hits — and from the truth's own history
(tests/temporal_truth.py and its motion and moments forms); never from the library's read-outs.  Everything is compared bit for bit.
tiny0 100x75: 4 x 3 blocks, both edge blocks partial, the width no multiple of 32, four blocks of sky."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import _native as N  # noqa: E402
from tests import history_reach_truth as HT  # noqa: E402
from tests import moments_truth as MT  # noqa: E402
from tests import temporal_truth as TT  # noqa: E402
from tests import test_gpu_denoise_motion as M  # noqa: E402    (its moved box and what the oracle says about it)
from tests import test_gpu_denoise_temporal as TG  # noqa: E402  (its camera sequence)
from tests import test_gpu_noise as G  # noqa: E402
from tests.helpers import bits  # noqa: E402

CASE = G.CASES[0]
W, H = CASE[1:3]
SPP = TG.SPP
F = np.float32
PLAN = dict(target=12, min_spp=2, max_spp=16, step=4)
same = TG.same


def plan_and_check(p, call, hist, tag, motion=None, **kw):
    """PlanByHistory at 0 spp against the truth: the reach, the bins, the plan and what the call reports.  call = (.., A, N, P, hit) of the oracle."""
    A, Nn, P, hit = call[3:7]
    args = dict(PLAN, **kw)
    cap = args.get("history_cap", 64.0)
    want_reach = HT.reach(Nn, P, A, hit, hist, cap) if motion is None else HT.reach_motion(Nn, P, A, hit, hist, motion[0], motion[1], motion[2], cap)
    want_bins = HT.bins(want_reach, hit)
    want_plan = HT.plan(want_bins, args["target"], args["min_spp"], args["max_spp"], args["step"], args.get("tolerance_permille", 31))
    info = p.PlanByHistory(**args)
    reach = p.ReadHistoryReach()
    assert same(reach, want_reach), "%s: %d words of the reach differ from the truth" % (tag, int((bits(reach) != bits(want_reach)).sum()))
    idx, got_bins = p.ReadHistoryBins()
    assert np.array_equal(idx, np.arange(len(want_bins))) and np.array_equal(got_bins, want_bins), tag + ": the bins"
    assert np.array_equal(got_bins.sum(1), [hit[ys, xs].sum() for _, ys, xs in HT.blocks_of(W, H)]), tag + ": the bins of a block do not sum to its hit pixels"
    idx, plan = p.ReadSamplePlan()
    assert np.array_equal(idx, np.arange(len(want_plan))) and np.array_equal(plan, want_plan), "%s: the plan %s, the truth's %s" % (tag, plan, want_plan)
    floors = HT.reach_bin(want_reach[hit])
    assert info["blocks"] == 12 and info["want_min"] == want_plan.min() and info["want_max"] == want_plan.max() and info["spp"] == 0 and info["pixels"] == W * H, info
    assert info["pixels_with_history"] == int((floors >= 1).sum()) and info["pixel_samples"] == HT.pixel_samples(want_plan, W, H), info
    assert abs(info["mean_reach"] - floors.sum() / (W * H)) < 1e-12 and info["reach_ms"] > 0.0 and info["capture_ms"] > 0.0, info
    assert info["device_bytes"] >= 12 * (4 * 1024 + 260), info
    assert p.GetSPP() == 0 and (p.ReadBlockSPP()[1] == 0).all(), tag + ": the plan traced or froze something"
    return want_reach, want_plan


def test_two_committed_poses_then_the_plan_of_the_third(scene_cache, sobol_matrices):
    inst, _ = G._instance(scene_cache, CASE)
    p, cfg = inst.m_path_tracer, inst.m_config
    p.SetNoiseStats(True)
    poses = TG.sequence(inst, CASE, sobol_matrices)
    # no denoiser at all, then no history: all zeros, and every block with a hit pixel gets the first candidate at or above the target
    pos, yaw, seed, call, cam = poses[0][:5]
    TG.set_pose(p, cfg, pos, yaw, seed, 0)
    for tag in ("no denoiser yet", "again"):
        reach, plan = plan_and_check(p, call, None, tag)
        assert not reach.any() and set(plan) == {2, 14}, plan  # (2: a block of sky; 14: the first of 2, 6, 10, 14, 16 at or above 12)
    hist = None
    for k in (0, 1):
        pos, yaw, seed, call, cam = poses[k][:5]
        TG.set_pose(p, cfg, pos, yaw, seed)
        _, _, hist = TT.denoise(*call, hist, cam)
        p.Denoise(temporal=True)
    pos, yaw, seed, call, cam = poses[2][:5]
    TG.set_pose(p, cfg, pos, yaw, seed, 0)
    reach, plan = plan_and_check(p, call, hist, "the third pose")
    hit = call[6]
    assert (reach[hit] > 0).mean() > 0.5 and F(SPP) < reach.max() <= F(2 * SPP) and len(set(plan)) >= 3, (float((reach[hit] > 0).mean()), reach.max(), plan)
    # other arguments: a cap below the lengths, a tolerance of 0 and a wide one, a step off the grid
    low, _ = plan_and_check(p, call, hist, "cap 2.5", history_cap=2.5)
    assert low.max() == F(2.5)
    _, strict = plan_and_check(p, call, hist, "tolerance 0", tolerance_permille=0)
    _, loose = plan_and_check(p, call, hist, "tolerance 500", tolerance_permille=500)
    assert (strict >= plan).all() and (loose <= plan).all() and strict.sum() > loose.sum()
    plan_and_check(p, call, hist, "step 3, max 13", step=3, max_spp=13)
    # what the merge then finds is the block's count and the reach: here after a uniform 4 spp
    p.Trace(True, SPP)
    p.Denoise(temporal=True, commit=False)
    assert same(p.ReadDenoiseHistory(), np.where(reach > 0, F(SPP) + reach, F(SPP)).astype(np.float32)), "the merge found another length than the plan foresaw"
    # a history of the other kind counts as none; so does none after ResetDenoiseHistory()
    TG.set_pose(p, cfg, pos, yaw, seed, 0)
    none, _ = plan_and_check(p, call, None, "a plain history asked for by a moments plan", moments=True)
    assert not none.any()
    plan_and_check(p, call, hist, "the plain history is still there")
    p.ResetDenoiseHistory()
    none, _ = plan_and_check(p, call, None, "after ResetDenoiseHistory()")
    assert not none.any()
    p.destroy()


def test_a_moments_history(scene_cache, sobol_matrices):
    inst, _ = G._instance(scene_cache, CASE)
    p, cfg = inst.m_path_tracer, inst.m_config
    p.SetNoiseStats(True)
    poses = TG.sequence(inst, CASE, sobol_matrices)
    pos, yaw, seed, call, cam = poses[0][:5]
    TG.set_pose(p, cfg, pos, yaw, seed)
    p.Denoise(temporal=True, moments=True)
    _, _, hist, _ = MT.denoise(*call, None, cam)
    pos, yaw, seed, call, cam = poses[1][:5]
    TG.set_pose(p, cfg, pos, yaw, seed, 0)
    reach, _ = plan_and_check(p, call, MT.history_for(hist, True), "moments=True on a moments history", moments=True)
    assert (reach[call[6]] > 0).mean() > 0.5
    none, _ = plan_and_check(p, call, MT.history_for(hist, False), "a plain plan on a moments history")
    assert not none.any()
    p.Trace(True, SPP)
    p.Denoise(temporal=True, moments=True, commit=False)
    assert same(p.ReadDenoiseHistory(), np.where(reach > 0, F(SPP) + reach, F(SPP)).astype(np.float32))
    p.destroy()


def test_after_a_pose_with_follow_motion(scene_cache, sobol_matrices):
    w = M.world(scene_cache, sobol_matrices)
    inst, _, _, _ = M.instance(scene_cache)
    p, cfg = inst.m_path_tracer, inst.m_config
    M.commit_rest(p, cfg, w)
    p.UpdateTriangles(0, w["moved"]["p"].reshape(-1, 9))
    pose = w["box_moved"]
    TG.set_pose(p, cfg, pose["pos"], pose["yaw"], pose["seed"], 0)
    cur = M.words(w["moved"])
    reach, _ = plan_and_check(p, pose["call"], w["hist"], "follow_motion", motion=(pose["tri"], pose["uv"], cur), follow_motion=True)
    still, _ = plan_and_check(p, pose["call"], w["hist"], "the still form on moved geometry")
    on_moved = np.isin(pose["tri"], w["box_ids"])
    assert on_moved.sum() > 50 and (reach[on_moved] > 0).mean() > 0.5 and not still[on_moved].any(), "the case: the moved box keeps its history only when it is followed"
    p.Trace(True, SPP)
    p.Denoise(temporal=True, follow_motion=True, commit=False)
    assert same(p.ReadDenoiseHistory(), np.where(reach > 0, F(SPP) + reach, F(SPP)).astype(np.float32))
    # a history without a snapshot (a committing call without follow_motion): every pixel is unmoved, the motion form is the still one
    p.Denoise(temporal=True)
    _, _, plain = TT.denoise(*pose["call"], w["hist"], pose["cam"])
    TG.set_pose(p, cfg, pose["pos"], pose["yaw"], pose["seed"], 0)
    plan_and_check(p, pose["call"], plain, "follow_motion without a snapshot", motion=(pose["tri"], pose["uv"], cur), follow_motion=True)
    p.destroy()


def test_read_outs_before_the_first_plan(scene_cache):
    inst, _ = G._instance(scene_cache, CASE)
    p = inst.m_path_tracer
    r = np.zeros((H, W), np.float32)
    assert N.lib.adypt_read_history_reach(p._ctx, r.ctypes.data) == N.E_STATE and b"no plan has been made yet" in N.lib.adypt_last_error(p._ctx)
    assert N.lib.adypt_read_sample_plan(p._ctx, None, None, 0) == N.E_STATE and N.lib.adypt_read_history_bins(p._ctx, None, None, 0) == N.E_STATE
    assert N.lib.adypt_read_history_reach(p._ctx, None) == N.E_INVALID and N.lib.adypt_read_sample_plan(p._ctx, None, None, -1) == N.E_INVALID
    p.destroy()
