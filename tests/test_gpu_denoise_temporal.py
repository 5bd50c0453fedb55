"""-m gpu: the denoiser's temporal merge (include/adypt_hip.h adypt_denoise_temporal ...; csrc/device/temporal.hpp, k_temporal_merge in denoise.hip).
The truth is computed in this process by the numpy restatement of the definition (tests/temporal_truth.py, tests/denoise_truth.py) from what the CPU
ORACLE gives for every pose — its image, the moments of its exact per-frame samples, its primary frames of types 0 / 4 / 5 — never from the library's
read-outs; the history of the truth is the truth's own.  Everything is compared bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import noise_truth as T  # noqa: E402
from tests import temporal_truth as TT  # noqa: E402
from tests import test_gpu_adaptive as A  # noqa: E402  (its schedule construction and its cached oracle runs)
from tests import test_gpu_denoise as DN  # noqa: E402  (its state snapshots and its truth of a call without history)
from tests import test_gpu_noise as G  # noqa: E402     (its cases)
from tests.helpers import bits, oracle_scene_from_instance  # noqa: E402
from tests.test_gpu_parity import make_instance  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "adypt_amd", "adypt_hip")
SEED = 31
SPP = 4
F = np.float32
CASES = G.CASES  # tiny0 100x75 (partial blocks on two edges), tiny0 96x64 (exact blocks), sibenik 160x90
IDS = ["%s-%dx%d" % c[:3] for c in CASES]
STEP_YAW, STEP_MOVE = 1.5, 0.15  # a step of the camera, as in tests/test_temporal_definition.py: a few pixels of motion at these sizes
AXIS = {"tiny0": 0, "sibenik": 2}
_poses = {}


def camera_of(c, name, k):
    """(position, yaw) of the case's camera k steps on"""
    pos = [float(v) for v in c.position]
    pos[AXIS[name]] += STEP_MOVE * k
    return pos, c.yaw + STEP_YAW * k


def oracle_pose(key, osc, c, pos, yaw, seed, sobol_matrices, frames=SPP):
    """What the oracle gives for one pose: (the filter's inputs after SPP frames, (origin, inv_proj, inv_view), the image after every frame); once per key."""
    if key not in _poses:
        w, h = c.width, c.height
        ip, iv = O.camera(c.fov, yaw, c.pitch, w, h)
        P = O.make_params(w, h, pos, ip, iv, stack_size=c.stack_size, max_bounce=c.max_bounce, subpixel=c.subpixel, tmp_life=c.tmp_lifetime, tmin=c.ray_tmin,
                          clamp=c.clamp, sun=list(c.sun))
        shift = O.shift_bytes(seed, w, h)
        samples = T.frame_samples(osc, P, shift, sobol_matrices, SPP)
        _, m2 = T.moments(samples)
        state, images = O.PathTracerState(w, h), []
        for _ in range(frames):
            O.pt_frames(osc, P, shift, sobol_matrices, state, 1)
            images.append(state.accum[..., :3].copy())
        g = [O.primary_frame(osc, P, t) for t in (0, 4, 5)]
        tri = g[0][1]["tri_id"].copy()
        call = (images[SPP - 1], m2, SPP, g[0][0][..., :3].copy(), g[1][0][..., :3].copy(), g[2][0][..., :3].copy(), tri != -1)
        _poses[key] = (call, (np.array(pos, np.float32), ip, iv), images, tri)
    return _poses[key]


def set_pose(t, cfg, pos, yaw, seed, spp=SPP):
    """the tracer at 0 spp under the camera and the seed given, then spp frames"""
    c = cfg.c
    t.Reset()
    t.SetConfig(cfg.pt_params(seed))
    ip, iv = api.camera_matrices(c.fov, yaw, c.pitch, c.width, c.height)
    t.SetCamera(ip, iv, np.array(pos, np.float32))
    if spp:
        t.Trace(True, spp)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def sequence(inst, case, sobol_matrices, n=3):
    """the oracle's poses of the case's first n cameras, each with a seed of its own"""
    c, osc = inst.m_config.c, oracle_scene_from_instance(inst)
    out = []
    for k in range(n):
        pos, yaw = camera_of(c, case[0], k)
        out.append((pos, yaw, SEED + k) + oracle_pose(case[:5] + (k,), osc, c, pos, yaw, SEED + k, sobol_matrices, frames=SPP + 2))
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_three_cameras_are_bit_exact_and_nothing_else_moves(case, scene_cache, sobol_matrices):
    inst, _ = G._instance(scene_cache, case)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    hist = None
    for k, (pos, yaw, seed, call, cam, images, _) in enumerate(sequence(inst, case, sobol_matrices)):
        set_pose(p, inst.m_config, pos, yaw, seed)
        assert same(p.ReadResult(), images[SPP - 1]), "camera %d: the image is not the oracle's" % k
        before, hits_before = DN.state_of(p), p.ReadHits()
        want, want_n, new = TT.denoise(*call, hist, cam)
        if k == 0:
            plain = p.Denoise()
        if k == 1:
            # the history is only read: two calls give the same bits, and the committing call after them what it would have given without them
            a, na = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
            b, nb = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
            assert same(a, want) and same(b, want) and same(na, want_n) and same(nb, want_n), "commit=False"
        got = p.Denoise(temporal=True)
        assert same(got, want), "camera %d: %d words of the result differ" % (k, int((bits(got) != bits(want)).sum()))
        assert same(p.ReadDenoiseHistory(), want_n), "camera %d: the history length" % k
        if k == 0:
            assert same(got, plain) and (want_n == F(SPP)).all(), "the first call is not Denoise()"
        else:
            took = want_n[call[6]] > F(SPP)
            assert took.mean() > 0.5, "camera %d: the case merges next to nothing (%.2f)" % (k, took.mean())
        assert p.GetDenoiseMergeMs() > 0.0 and len(p.GetDenoiseTiming()["levels"]) == 5
        DN.assert_same_state(DN.state_of(p), before, "around Denoise(temporal=True) at camera %d" % k)
        hits_after = p.ReadHits()
        assert np.array_equal(hits_after[0], hits_before[0]) and same(hits_after[1], hits_before[1]), "the primary-hit cache moved"
        hist = new
    p.Trace(True, 2)
    assert p.GetSPP() == SPP + 2 and same(p.ReadResult(), images[SPP + 1]), "tracing on after the temporal calls left the oracle's image"
    p.destroy()


def test_plain_denoise_between_two_temporal_calls_changes_nothing(scene_cache, sobol_matrices):
    case = CASES[1]
    inst, _ = G._instance(scene_cache, case)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    poses = sequence(inst, case, sobol_matrices)
    pos, yaw, seed, call0, cam0 = poses[0][:5]
    set_pose(p, inst.m_config, pos, yaw, seed)
    p.Denoise(temporal=True)
    _, _, hist = TT.denoise(*call0, None, cam0)
    pos, yaw, seed, call, cam = poses[1][:5]
    set_pose(p, inst.m_config, pos, yaw, seed)
    a, na = p.Denoise(temporal=True, commit=False, history_cap=8.0), p.ReadDenoiseHistory()
    plain = p.Denoise(levels=3)
    assert same(plain, DN.D.denoise(*call, levels=3)), "Denoise() read the history"
    assert same(p.ReadDenoiseHistory(), na), "Denoise() moved the history length"
    b, nb = p.Denoise(temporal=True, commit=False, history_cap=8.0), p.ReadDenoiseHistory()
    want, want_n, _ = TT.denoise(*call, hist, cam, cap=8.0)
    assert same(a, want) and same(b, want) and same(na, want_n) and same(nb, want_n)
    # a cap below n, and other filter parameters
    want, want_n, _ = TT.denoise(*call, hist, cam, cap=2.5, levels=2, sigma_l=2.0, sigma_z=0.3)
    assert same(p.Denoise(2, 2.0, 0.3, temporal=True, history_cap=2.5, commit=False), want) and same(p.ReadDenoiseHistory(), want_n)
    assert (want_n <= F(SPP + 2.5)).all()
    # ResetDenoiseHistory(): the next call is the plain filter's bits, and commits
    p.ResetDenoiseHistory()
    got = p.Denoise(temporal=True)
    assert same(got, DN.D.denoise(*call)) and (p.ReadDenoiseHistory() == F(SPP)).all()
    again, n_again = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
    _, _, own = TT.denoise(*call, None, cam)
    want, want_n, _ = TT.denoise(*call, own, cam)
    assert same(again, want) and same(n_again, want_n) and (want_n[call[6]] > F(SPP)).mean() > 0.9  # (its own history, an unchanged camera)
    p.ResetDenoiseHistory()
    p.ResetDenoiseHistory()  # no error when there is none
    p.destroy()


# ---- moving geometry ----
MOVED_BOX = ((-1.8, 0.0, 1.0), (-1.2, 1.2, 1.6))  # the matte2 box of tiny0 (adypt_amd/scenes.py)
# moved by 0.3 along every axis: each of its faces moves 0.3 along its normal, the plane tolerance at its distance from the camera (about 5.5) is 0.11
MOVE = (0.3, 0.3, 0.3)
GEOMETRY = ("tiny0", 100, 75, 16, 1)  # no sub-pixel jitter: the primary-hit cache (ReadHits) holds the pixel-centre ray's hit, which the guides are of


def test_moved_geometry_starts_again_and_the_rest_keeps_its_history(scene_cache, sobol_matrices):
    name, w, h, life, sub = GEOMETRY
    spec = scenes.make_scene(name, scene_cache, width=w, height=h, pt={"tmpLifetime": life, "maxBounce": 6, "subpixel": sub, "stackSize": 32})
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=SEED), api.InstanceConfig.last_error()
    p, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    p.SetNoiseStats(True)
    tris = np.array(inst.scene.triangles).view(O.TRI_DT)
    lo, hi = np.array(MOVED_BOX[0]) - 1e-4, np.array(MOVED_BOX[1]) + 1e-4
    on_box = ((tris["p"] >= lo) & (tris["p"] <= hi)).all(axis=(1, 2))
    assert on_box.sum() == 12
    moved = tris.copy()
    moved["p"][on_box] += np.array(MOVE, np.float32)

    def oracle_scene(t):
        b = api.WideBVH()
        b.BuildPLOC(api.Scene.FromArrays(t, inst.scene.materials), cfg.bvh_params(), 8, 0.0)
        return O.Scene(b.nodes, b.tri_indices, np.ascontiguousarray(t).view(np.uint8).reshape(-1), inst.scene.materials, textures=inst.scene.textures)

    # the rest pose, committed
    pos0, yaw0 = camera_of(c, name, 0)
    call0, cam0, _, tri0 = oracle_pose(("geometry", "rest"), oracle_scene_from_instance(inst), c, pos0, yaw0, SEED, sobol_matrices)
    set_pose(p, cfg, pos0, yaw0, SEED)
    assert np.array_equal(p.ReadHits()[0], tri0)
    got = p.Denoise(temporal=True)
    want, _, hist = TT.denoise(*call0, None, cam0)
    assert same(got, want)
    # the box moves, the camera goes a step on; the history is only read from here on
    pos1, yaw1 = camera_of(c, name, 1)
    call1, cam1, _, tri1 = oracle_pose(("geometry", "moved"), oracle_scene(moved), c, pos1, yaw1, SEED + 1, sobol_matrices)
    want, want_n, _ = TT.denoise(*call1, hist, cam1)
    box_ids = np.nonzero(on_box)[0]

    def check(tag):
        set_pose(p, cfg, pos1, yaw1, SEED + 1)
        assert same(p.ReadResult(), call1[0]), tag + ": the image is not the oracle's"
        hits = p.ReadHits()[0]
        assert np.array_equal(hits, tri1), tag
        got, n_out = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
        assert same(got, want) and same(n_out, want_n), tag
        on_moved = np.isin(hits, box_ids)
        assert on_moved.sum() > 50 and (n_out[on_moved] == F(SPP)).all(), tag + ": a pixel on a moved triangle took history"
        static = (hits >= 0) & ~on_moved
        assert (n_out[static] > F(SPP)).mean() > 0.8, tag + ": the static pixels lost their history"

    p.UpdateTriangles(0, moved["p"].reshape(-1, 9))
    check("after UpdateTriangles")
    p.RebuildBVH(method="ploc")
    check("after RebuildBVH(method='ploc')")
    # the box removed: what it hid starts again where the history holds the box, bit for bit as numpy says
    without = np.ascontiguousarray(tris[~on_box])
    call2, cam2, _, tri2 = oracle_pose(("geometry", "removed"), oracle_scene(without), c, pos1, yaw1, SEED + 2, sobol_matrices)
    p.SetTriangles(without.view(np.uint8).reshape(-1))
    set_pose(p, cfg, pos1, yaw1, SEED + 2)
    assert same(p.ReadResult(), call2[0]) and np.array_equal(p.ReadHits()[0], tri2)
    got, n_out = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
    want2, want_n2, _ = TT.denoise(*call2, hist, cam2)
    assert same(got, want2) and same(n_out, want_n2)
    ok, fx, fy, _ = TT.reproject(hist["cam"], w, h, call2[5])
    ix, iy = np.floor(np.where(ok, fx, 0)).astype(int), np.floor(np.where(ok, fy, 0)).astype(int)
    inside = ok & call2[6] & (ix >= 0) & (iy >= 0) & (ix < w - 1) & (iy < h - 1)
    ixc, iyc = np.clip(ix, 0, w - 2), np.clip(iy, 0, h - 2)
    was_box = np.isin(tri0, box_ids)
    behind_box = inside & was_box[iyc, ixc] & was_box[iyc, ixc + 1] & was_box[iyc + 1, ixc] & was_box[iyc + 1, ixc + 1]
    assert behind_box.sum() > 50 and (n_out[behind_box] == F(SPP)).all(), "a pixel that looks at where the box was took the box's history"
    assert (n_out[call2[6] & ~behind_box] > F(SPP)).mean() > 0.8
    p.destroy()


def test_adaptive_blocks_at_their_own_sample_counts(scene_cache, sobol_matrices):
    """tiny0 100x75: a uniform pose a step away is committed, then the adaptive run of tests/test_gpu_denoise.py (blocks frozen at 8 ... and one still
    active) merges it with n per block and commits; a third pose reads a history whose lengths differ per block."""
    case = A.TINY0
    name, w, h, life, sub, every, min_spp, cap, nominal = case
    inst, _ = A._instance(scene_cache, case)
    p, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    osc = oracle_scene_from_instance(inst)
    samples, images = A._truth(inst, case, sobol_matrices)
    table, target, spp_b, counter, frozen = A.plan_of(case, samples)
    spp32, counter32, frozen32 = A.schedule(table, target, every, min_spp, 32)
    assert 0 < len(frozen32) < len(spp32) and len(set(spp32.tolist())) >= 3
    p.SetNoiseStats(True)
    pos1, yaw1 = camera_of(c, name, 1)
    call1, cam1, _, _ = oracle_pose(case[:5] + ("adaptive", 1), osc, c, pos1, yaw1, A.SEED + 1, sobol_matrices)
    set_pose(p, cfg, pos1, yaw1, A.SEED + 1)
    want, _, hist = TT.denoise(*call1, None, cam1)
    assert same(p.Denoise(temporal=True), want)
    pos0, yaw0 = camera_of(c, name, 0)
    set_pose(p, cfg, pos0, yaw0, A.SEED, spp=0)
    p.TraceAdaptive(target, min_spp, 32, every)
    before = DN.state_of(p)
    assert np.array_equal(before["block_spp"], spp32)
    exp = A.expected(samples, images, w, h, spp32)
    g = DN.guides_of(inst, case)
    call0 = (exp["image"], exp["moments"][..., 1], spp32, g["albedo"], g["normal"], g["position"], g["hit"])
    ip, iv = O.camera(c.fov, yaw0, c.pitch, w, h)
    want, want_n, hist = TT.denoise(*call0, hist, (np.array(pos0, np.float32), ip, iv))
    got = p.Denoise(temporal=True)
    assert same(got, want) and same(p.ReadDenoiseHistory(), want_n), "blocks at their own counts"
    assert len(np.unique(want_n[~g["hit"]])) >= 3  # (sky pixels: n_out is the block's own count)
    DN.assert_same_state(DN.state_of(p), before, "around Denoise(temporal=True) with blocks frozen")
    set_pose(p, cfg, pos1, yaw1, A.SEED + 1)
    want, want_n, _ = TT.denoise(*call1, hist, cam1)
    assert same(p.Denoise(temporal=True), want) and same(p.ReadDenoiseHistory(), want_n), "a history of per-block lengths"
    p.destroy()


@pytest.mark.parametrize("shape,n_dev", [((100, 75), 2), ((100, 75), 3), ((96, 64), 4), ((64, 36), 4)], ids=["100x75-2", "100x75-3", "96x64-4", "64x36-4-one-owns-nothing"])
def test_multi_device_on_one_card(shape, n_dev, scene_cache, monkeypatch):
    """Several shards on one card against one context over two committing calls: identical bits (the one-context bits are held against numpy above)."""
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    w, h = shape
    case = ("tiny0", w, h, 16, 3, SPP)
    inst, _ = G._instance(scene_cache, case)
    single, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    m = api.MultiPathTracer()
    m.Initialize(cfg.pt_params(SEED), inst.m_hipscene, c.width, c.height, (0,) * n_dev)
    assert m.DeviceCount() == n_dev
    if shape == (64, 36):
        assert any(N.lib.adypt_local_pixel_count(x) == 0 for x in m._contexts())
    for t in (single, m):
        t.SetNoiseStats(True)
    for k in range(2):
        pos, yaw = camera_of(c, "tiny0", k)
        out = []
        for t in (single, m):
            set_pose(t, cfg, pos, yaw, SEED + k)
            out.append((t.Denoise(temporal=True), t.ReadDenoiseHistory(), t.ReadResult()))
        assert same(out[0][2], out[1][2]), "the images differ"
        assert same(out[0][0], out[1][0]), "call %d: %d shards against one context" % (k, n_dev)
        assert same(out[0][1], out[1][1]), "call %d: the history length" % k
    assert (out[1][1] > F(SPP)).mean() > 0.3 and m.GetDenoiseMergeMs() > 0.0
    m.ResetDenoiseHistory()
    assert same(m.Denoise(temporal=True, commit=False), single.Denoise())
    # a shard context refuses the per-context call
    with pytest.raises(N.AdyptError) as e:
        N.check(N.lib.adypt_denoise_temporal(m._contexts()[0], None, None), m._contexts()[0])
    assert e.value.code == N.E_STATE and "tile shard" in str(e.value)
    m.destroy()
    single.destroy()


def test_refusals(scene_cache):
    inst = make_instance(scene_cache, "tiny0", 96, 64)
    p = inst.m_path_tracer
    length = np.zeros((64, 96), np.float32)

    def refused(code, word, **kw):
        with pytest.raises(N.AdyptError) as e:
            p.Denoise(temporal=True, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)
    assert N.lib.adypt_read_denoise_history(p._ctx, length.ctypes.data) == N.E_STATE and b"no temporal call" in N.lib.adypt_last_error(p._ctx)
    assert N.lib.adypt_denoise_history_reset(p._ctx) == N.ADYPT_OK  # nothing to drop: no error
    p.Trace(True, 4)
    refused(N.E_STATE, "statistics are off")
    p.Reset()
    p.SetNoiseStats(True)
    p.Trace(True, 1)
    refused(N.E_STATE, "at least 2 spp")
    p.Trace(True, 1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(N.E_INVALID, "history_cap must be a positive finite number", history_cap=bad)
    refused(N.E_INVALID, "levels must be in [1, 6]", levels=7)
    assert N.lib.adypt_read_denoise_history(p._ctx, length.ctypes.data) == N.E_STATE  # the refused calls left nothing
    plain = p.Denoise()
    assert N.lib.adypt_read_denoise_history(p._ctx, length.ctypes.data) == N.E_STATE  # nor does Denoise()
    with pytest.raises(N.AdyptError):
        p.GetDenoiseMergeMs()
    assert N.lib.adypt_denoise_temporal(p._ctx, None, None) == N.ADYPT_OK  # null pointers: the defaults (cap 64, committing)
    assert not same(p.Denoise(temporal=True, commit=False), plain)  # (its own history under an unchanged camera: merged)
    assert N.lib.adypt_read_denoise_history(p._ctx, length.ctypes.data) == N.ADYPT_OK and (length >= 2).all() and (length > 2).any()
    p.Trace(False)
    refused(N.E_STATE, "not path-traced")
    p.destroy()
    part = make_instance(scene_cache, "tiny0", 100, 75, rank=1, world=2)
    q = part.m_path_tracer
    q.SetNoiseStats(True)
    q.Trace(True, 3)
    with pytest.raises(N.AdyptError) as e:
        q.Denoise(temporal=True)
    assert e.value.code == N.E_STATE and "tile shard" in str(e.value)
    q.destroy()


@pytest.mark.parametrize("n_dev", [1, 2], ids=["one-context", "2-shards"])
def test_read_outs_follow_the_call_sequence(n_dev, scene_cache, monkeypatch):
    """tiny0 96x64 at 2 spp: after every step of a sequence of accepted and refused calls, which of the five read-outs answer and which return
    E_STATE, and that what answers is, bit for bit, what the same read-out gave right after the call that produced it."""
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    inst = make_instance(scene_cache, "tiny0", 96, 64)
    t = inst.m_path_tracer
    if n_dev > 1:
        t = api.MultiPathTracer()
        t.Initialize(inst.m_config.pt_params(SEED), inst.m_hipscene, 96, 64, (0,) * n_dev)
        assert t.DeviceCount() == n_dev
    t.SetNoiseStats(True)
    set_pose(t, inst.m_config, *camera_of(inst.m_config.c, "tiny0", 0), SEED, spp=2)

    def read_denoised():
        rgb = np.zeros((64, 96, 3), F)
        t._call("read_denoised", rgb.ctypes.data)
        return rgb
    reads = {"denoised": read_denoised, "length": t.ReadDenoiseHistory, "motion": t.ReadDenoiseMotion}
    kept = {}  # what a read-out gave right after the call that produced it

    def step(tag, denoised, length, motion, merge, levels):
        """every column: "new" (answers; kept from here on), "kept" (answers with the kept bits) or None (E_STATE); merge: answers (> 0) or not"""
        for name, want in (("denoised", denoised), ("length", length), ("motion", motion)):
            if want is None:
                with pytest.raises(N.AdyptError) as e:
                    reads[name]()
                assert e.value.code == N.E_STATE, "%s: %s" % (tag, name)
                continue
            got = reads[name]()
            got = np.concatenate([got["previous_position"].reshape(-1), got["moved"].astype(F).reshape(-1)]) if name == "motion" else got
            if want == "new":
                kept[name] = got
            assert same(got, kept[name]), "%s: %s is not what it was after the call that produced it" % (tag, name)
        if merge:
            assert t.GetDenoiseMergeMs() > 0.0, tag
        else:
            with pytest.raises(N.AdyptError) as e:
                t.GetDenoiseMergeMs()
            assert e.value.code == N.E_STATE, "%s: merge ms" % tag
        if levels is None:
            with pytest.raises(N.AdyptError) as e:
                t.GetDenoiseTiming()
            assert e.value.code == N.E_STATE, "%s: timing" % tag
        else:
            assert len(t.GetDenoiseTiming()["levels"]) == levels, "%s: timing entries" % tag

    def refused(**kw):
        with pytest.raises(N.AdyptError) as e:
            t.Denoise(**kw)
        assert e.value.code == N.E_INVALID, str(e.value)
    step("nothing yet", None, None, None, False, None)
    plain = t.Denoise()
    step("Denoise()", "new", None, None, False, 5)
    assert same(kept["denoised"], plain)
    a = t.Denoise(temporal=True, commit=False)
    step("temporal, commit = 0", "new", "new", None, True, 5)
    assert same(kept["denoised"], a) and same(a, plain) and (kept["length"] == F(2)).all()  # (no history: the plain filter)
    b = t.Denoise(temporal=True, commit=False, follow_motion=True)
    step("motion, commit = 0", "new", "new", "new", True, 5)
    assert same(kept["denoised"], b)
    c = t.Denoise(temporal=True, commit=False)
    step("temporal, commit = 0, again", "new", "new", "kept", True, 5)
    assert same(kept["denoised"], c)
    three = t.Denoise(levels=3)
    step("Denoise(levels=3)", "new", "kept", "kept", False, 3)
    assert same(kept["denoised"], three) and not same(three, plain)
    refused(levels=7)
    refused(temporal=True, history_cap=0.0)
    step("refused calls", "kept", "kept", "kept", False, 3)
    t.ResetDenoiseHistory()
    step("history reset", "kept", "kept", "kept", False, 3)
    last = t.Denoise(temporal=True)
    step("temporal, committing", "new", "new", "kept", True, 5)
    assert same(kept["denoised"], last) and same(last, plain) and (kept["length"] == F(2)).all()
    if n_dev > 1:
        t.destroy()
    inst.m_path_tracer.destroy()


def test_cli(scene_cache, sobol_matrices, tmp_path):
    """Two --history-from configs on tiny0 96x64 against the same sequence through Python."""
    case = CASES[1]
    name, w, h = case[:3]
    inst, spec = G._instance(scene_cache, case)
    p, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    p.SetNoiseStats(True)
    main = json.load(open(spec.config_path))
    paths = []
    for k in (1, 2):  # the earlier poses: two and one step away from the main config's camera
        pos, yaw = camera_of(c, name, 3 - k)
        other = json.loads(json.dumps(main))
        other["camera"]["position"], other["camera"]["yaw"] = pos, yaw
        paths.append(str(tmp_path / ("pose%d.config" % k)))
        json.dump(other, open(paths[-1], "w"), indent=4)
        check = api.InstanceConfig()
        assert check.LoadFromFile(paths[-1]), api.InstanceConfig.last_error()
        assert check.c.yaw == F(yaw) and list(check.c.position) == [F(v) for v in pos]
        set_pose(p, cfg, pos, yaw, SEED + k)
        p.Denoise(temporal=True, history_cap=16.0)
    pos, yaw = camera_of(c, name, 0)
    set_pose(p, cfg, pos, yaw, SEED)
    img, den, length, hit = p.ReadResult(), p.Denoise(temporal=True, history_cap=16.0), p.ReadDenoiseHistory(), p.ReadDenoiseGuides()["hit"]
    p.destroy()
    out, d_exr, l_exr = str(tmp_path / "o.exr"), str(tmp_path / "d.exr"), str(tmp_path / "l.exr")
    copy = str(tmp_path / "main.config")  # (the tool writes its config back on exit)
    json.dump(main, open(copy, "w"), indent=4)

    def cli(*args):
        r = subprocess.run([CLI, copy, "--out", out, "--seed", str(SEED), "--spp", str(SPP)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        return r.returncode, (r.stdout + r.stderr).decode()
    code, text = cli("--denoise", d_exr, "--history-from", paths[0], "--history-from", paths[1], "--history-cap", "16", "--history-out", l_exr)
    assert code == 0 and "Saved denoised image (5 levels)" in text, text[-2000:]
    assert same(api.load_exr(out), img) and same(api.load_exr(d_exr), den), "the tool's images are not the Python sequence's"
    assert same(api.load_exr(l_exr)[..., 0], length)
    took = int((length[hit] > SPP).sum())
    line = "[PT]TEMPORAL: history on %d of %d hit pixels, mean length %.3f" % (took, int(hit.sum()), float(length[hit].astype(np.float64).mean()))
    assert line in text, text[-2000:]
    assert took > 0.5 * hit.sum()
    # (a config of another size, the history options without --denoise, a cap that is no positive finite number: tests/test_cli_options.py)
