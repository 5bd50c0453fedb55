"""-m gpu: variance from temporal moments (include/adypt_hip.h adypt_denoise_temporal_moments ...; csrc/device/moments.hpp, k_denoise_prepare_moments,
k_temporal_merge_moments and k_moments_variance in denoise.hip).  The truth is computed in this process by the numpy restatement of the definition
(tests/moments_truth.py) from what the CPU ORACLE gives for every pose at 1 spp — its image, the moments of its exact per-frame samples, its primary
frames of types 0 / 4 / 5 — never from the library's read-outs; the history of the truth is the truth's own.  Everything is compared bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import denoise_truth as D  # noqa: E402
from tests import moments_truth as MT  # noqa: E402
from tests import noise_truth as T  # noqa: E402
from tests import temporal_truth as TT  # noqa: E402
from tests import test_gpu_denoise as DN  # noqa: E402          (its state snapshots)
from tests import test_gpu_denoise_motion as M  # noqa: E402   (its moved box and what the oracle says about it)
from tests import test_gpu_denoise_temporal as TG  # noqa: E402 (its camera steps)
from tests.helpers import bits, oracle_scene_from_instance  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "adypt_amd", "adypt_hip")
SEED = TG.SEED
F = np.float32
#        scene      w    h  life sub
CASES = [("tiny0", 33, 9, 16, 3),      # one pixel past a workgroup (32 x 8) in x and in y: a tile's halo clips on all four sides of the image
         ("sibenik", 70, 20, 3, 1)]    # three workgroups by three: halos cross workgroup borders in both directions
IDS = ["%s-%dx%d" % c[:3] for c in CASES]
same = TG.same
N_POSES = 6
_poses = {}


def instance(scene_cache, case):
    name, w, h, life, sub = case
    spec = scenes.make_scene(name, scene_cache, width=w, height=h, pt={"tmpLifetime": life, "maxBounce": 6, "subpixel": sub})
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=SEED), api.InstanceConfig.last_error()
    inst.m_path_tracer.SetNoiseStats(True)
    return inst, spec


def oracle_pose(key, osc, c, k, seed, sobol_matrices, frames=2):
    """What the oracle gives for the case's camera k steps on: dict(pos, yaw, seed, calls {spp: the filter's inputs after spp frames}, cam, images (after
    every frame)); once per key."""
    key = key + (k, seed)
    if key not in _poses:
        pos, yaw = TG.camera_of(c, key[0], k)
        w, h = c.width, c.height
        ip, iv = O.camera(c.fov, yaw, c.pitch, w, h)
        P = O.make_params(w, h, pos, ip, iv, stack_size=c.stack_size, max_bounce=c.max_bounce, subpixel=c.subpixel, tmp_life=c.tmp_lifetime, tmin=c.ray_tmin,
                          clamp=c.clamp, sun=list(c.sun))
        shift = O.shift_bytes(seed, w, h)
        samples = T.frame_samples(osc, P, shift, sobol_matrices, frames)
        g = [O.primary_frame(osc, P, t) for t in (0, 4, 5)]
        tri = g[0][1]["tri_id"].copy()
        state, images, calls = O.PathTracerState(w, h), [], {}
        for spp in range(1, frames + 1):
            O.pt_frames(osc, P, shift, sobol_matrices, state, 1)
            images.append(state.accum[..., :3].copy())
            calls[spp] = (images[-1], T.moments(samples[:spp])[1], spp, g[0][0][..., :3].copy(), g[1][0][..., :3].copy(), g[2][0][..., :3].copy(), tri != -1)
        _poses[key] = dict(pos=pos, yaw=yaw, seed=seed, calls=calls, cam=(np.array(pos, np.float32), ip, iv), images=images)
    return _poses[key]


def sequence(inst, case, sobol_matrices):
    """the oracle's poses of the case's first three cameras, each with a seed of its own, and three more under the third's camera with seeds of their own"""
    c, osc = inst.m_config.c, oracle_scene_from_instance(inst)
    return [oracle_pose(case, osc, c, min(k, 2), SEED + k, sobol_matrices) for k in range(N_POSES)]


def go(t, cfg, pose, spp=1):
    TG.set_pose(t, cfg, pose["pos"], pose["yaw"], pose["seed"], spp)


def state_of(p):
    """tests/test_gpu_denoise.py's snapshot without the noise estimate, which needs 2 spp"""
    return dict(result=p.ReadResult(), moments=p.ReadNoiseMoments(), spp=p.GetSPP(), noise=None, ahead=p.GetLookaheadFrames(), block_spp=p.ReadBlockSPP()[1])


def moments_call(t, **kw):
    """(result, history length, variance, info) of one moments call"""
    return t.Denoise(temporal=True, moments=True, **kw), t.ReadDenoiseHistory(), t.ReadDenoiseVariance(), t.GetDenoiseMoments()


def assert_truth(got, want, tag):
    out, n_out, v, info = got
    w_out, w_n, _, extra = want
    assert same(out, w_out), "%s: %d words of the result differ" % (tag, int((bits(out) != bits(w_out)).sum()))
    assert same(n_out, w_n), "%s: %d words of the history length differ" % (tag, int((bits(n_out) != bits(w_n)).sum()))
    assert same(v, extra["V"]), "%s: %d words of the variance differ" % (tag, int((bits(v) != bits(extra["V"])).sum()))
    assert info["have"] == 1 and info["pixels_spatial"] == int(extra["spatial"].sum()), "%s: %s, the truth counts %d spatial pixels" % (tag, info, int(extra["spatial"].sum()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_three_poses_at_1_spp_and_more_under_the_same_camera(case, scene_cache, sobol_matrices):
    """Three poses at 1 spp, committing: the truth's bits in the result, the history length and the variance at every pose, and its count of spatial
    pixels — at the first pose every hit pixel whose window has 4 taps.  At 1 spp per pose no history is 4 samples long before the fourth pose, so by
    the definition every hit pixel still asks its window at the third (the truth counts 67 of 80 hit pixels on tiny0 33x9, 1368 of 1389 on sibenik
    70x20), and at the fourth pose under the third's camera the pixels whose history is shorter than the oldest's still do (2 and 435).  The sixth pose
    — the fourth under that camera, each with a seed of its own — is the first at which the truth says every hit pixel's history is at least 4 long:
    no pixel is spatial, the workgroup vote skipped every halo, and the bits are still the truth's."""
    inst, _ = instance(scene_cache, case)
    p, cfg = inst.m_path_tracer, inst.m_config
    w, h = case[1:3]
    hist, poses = None, sequence(inst, case, sobol_matrices)
    for k, pose in enumerate(poses):
        go(p, cfg, pose)
        call = pose["calls"][1]
        assert same(p.ReadResult(), call[0]), "pose %d: the image is not the oracle's" % k
        before, hits_before = state_of(p), p.ReadHits()
        want = MT.denoise(*call, hist, pose["cam"])
        hit, extra = call[6], want[3]
        if k == 1:
            # the history is only read: two calls give the same bits, and the committing call after them what it would have given without them
            assert_truth(moments_call(p, commit=False), want, "commit=False")
            assert_truth(moments_call(p, commit=False), want, "commit=False, again")
        got = moments_call(p)
        assert_truth(got, want, "pose %d" % k)
        info = got[3]
        assert info["variance_ms"] > 0.0 and info["device_bytes"] >= 4 * w * h + 512 and p.GetDenoiseMergeMs() >= info["variance_ms"] and len(p.GetDenoiseTiming()["levels"]) == 5, info
        DN.assert_same_state(state_of(p), before, "around the moments call at pose %d" % k)
        hits_after = p.ReadHits()
        assert np.array_equal(hits_after[0], hits_before[0]) and same(hits_after[1], hits_before[1]), "the primary-hit cache moved"
        print("%s pose %d: %d of %d hit pixels spatial, %d found history" % (IDS[CASES.index(case)], k, int(extra["spatial"].sum()), int(hit.sum()), int((want[1][hit] > F(1)).sum())))
        if k == 0:
            assert np.array_equal(extra["spatial"], hit & (extra["k"] >= F(4))) and extra["spatial"].sum() > 0.5 * hit.sum()
        if k == 2:
            assert (want[1][hit] < F(4)).all() and np.array_equal(extra["spatial"], hit & (extra["k"] >= F(4))) and (want[1][hit] > F(1)).mean() > 0.5
        if k == 3:
            assert extra["spatial"].any() and (want[1][hit] >= F(4)).any(), "the fourth pose: pixels on both sides of kMomentsMinLength"
        if k == N_POSES - 1:
            assert not extra["spatial"].any() and (want[1][hit] >= F(4)).all() and info["pixels_spatial"] == 0, "the last pose: a pixel asked its window"
        hist = want[2]
    p.Trace(True, 2)
    assert p.GetSPP() == 3 and p.ReadResult().shape == (h, w, 3)
    p.destroy()


def test_following_moved_geometry(scene_cache, sobol_matrices):
    """tests/test_gpu_denoise_motion.py's box at 1 spp: a committing moments call with follow_motion at rest, UpdateTriangles, then the call after — the
    truth's bits, and the moved box keeps its history."""
    w = M.world(scene_cache, sobol_matrices)

    def at_1_spp(name):
        pose = w[name]
        image = TG._poses[("geometry", {"rest": "rest", "box_moved": "moved"}[name])][2][0]  # (the oracle's image after the first frame)
        call = (image, T.moments(image[None])[1], 1) + tuple(pose["call"][3:])
        return dict(pose, call=call)
    rest, moved = at_1_spp("rest"), at_1_spp("box_moved")
    first = MT.denoise(*rest["call"], None, rest["cam"], motion=(rest["tri"], rest["uv"], M.words(w["tris"])))
    want = MT.denoise(*moved["call"], first[2], moved["cam"], motion=(moved["tri"], moved["uv"], M.words(w["moved"])))
    on_moved = np.isin(moved["tri"], w["box_ids"])
    assert (want[1][on_moved] > F(1)).mean() > 0.3, "the case: box pixels with history"
    inst, _, _, _ = M.instance(scene_cache)
    p, cfg = inst.m_path_tracer, inst.m_config
    TG.set_pose(p, cfg, rest["pos"], rest["yaw"], rest["seed"], 1)
    assert same(p.ReadResult(), rest["call"][0]), "the image is not the oracle's"
    assert_truth(moments_call(p, follow_motion=True), first, "the rest pose")
    assert p.GetDenoiseMotion()["have_snapshot"] == 1
    p.UpdateTriangles(0, w["moved"]["p"].reshape(-1, 9))
    TG.set_pose(p, cfg, moved["pos"], moved["yaw"], moved["seed"], 1)
    assert same(p.ReadResult(), moved["call"][0]), "the image is not the oracle's"
    got = moments_call(p, follow_motion=True, commit=False)
    assert_truth(got, want, "box moved")
    assert np.array_equal(p.ReadDenoiseMotion()["moved"], on_moved)
    # without follow_motion the box starts again
    got = moments_call(p, commit=False)
    assert_truth(got, MT.denoise(*moved["call"], first[2], moved["cam"]), "box moved, not followed")
    assert (got[1][on_moved] == F(1)).all()
    p.destroy()


def test_plain_calls_around_a_moments_call(scene_cache, sobol_matrices):
    """A plain Denoise() at 2 spp and a plain temporal call give exactly the bits their own truths give, before and after moments calls; neither kind finds
    the other's history; a committing call of either kind replaces it."""
    case = CASES[1]
    inst, _ = instance(scene_cache, case)
    p, cfg = inst.m_path_tracer, inst.m_config
    poses = sequence(inst, case, sobol_matrices)
    go(p, cfg, poses[0], 2)
    call2 = poses[0]["calls"][2]
    assert same(p.Denoise(), D.denoise(*call2))
    out, n_out, plain_hist = TT.denoise(*call2, None, poses[0]["cam"])
    assert same(p.Denoise(temporal=True), out) and same(p.ReadDenoiseHistory(), n_out)  # commits a plain history
    # a moments call on a plain history: none found; it commits its own
    go(p, cfg, poses[1])
    want = MT.denoise(*poses[1]["calls"][1], plain_hist, poses[1]["cam"])
    assert (want[1] == F(1)).all()
    assert_truth(moments_call(p), want, "a moments call on a plain call's history")
    variance = p.ReadDenoiseVariance()
    # the plain calls at 2 spp under the third camera: the plain filter's bits, and a temporal call that finds no history in the moments call's
    go(p, cfg, poses[2], 2)
    call2 = poses[2]["calls"][2]
    assert same(p.Denoise(), D.denoise(*call2)), "a plain Denoise() after a moments call"
    out, n_out, _ = TT.denoise(*call2, MT.history_for(want[2], False), poses[2]["cam"])
    assert MT.history_for(want[2], False) is None and (n_out == F(2)).all()
    assert same(p.Denoise(temporal=True, commit=False), out) and same(p.ReadDenoiseHistory(), n_out), "a plain temporal call after a committing moments call found history"
    assert same(p.ReadDenoiseVariance(), variance) and p.GetDenoiseMoments()["have"] == 1, "a plain call moved the variance read-out"
    # the moments call's history is still there for the next moments call
    go(p, cfg, poses[2])
    third = MT.denoise(*poses[2]["calls"][1], want[2], poses[2]["cam"])
    assert (third[1] > F(1)).any()
    assert_truth(moments_call(p), third, "a moments call after plain calls that did not commit")
    # a committing plain temporal call replaces it
    go(p, cfg, poses[2], 2)
    p.Denoise(temporal=True)
    go(p, cfg, poses[3])
    none = MT.denoise(*poses[3]["calls"][1], None, poses[3]["cam"])
    assert (none[1] == F(1)).all()
    assert_truth(moments_call(p, commit=False), none, "a moments call after a committing plain temporal call")
    p.destroy()


@pytest.mark.parametrize("n_dev", [2, 3])
def test_multi_device_on_one_card(n_dev, scene_cache, sobol_matrices, monkeypatch):
    """Several shards on one card against one context over the six committing moments calls of the sequence above: identical bits (the one-context bits are held against numpy above)."""
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = CASES[1]
    inst, _ = instance(scene_cache, case)
    single, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    m = api.MultiPathTracer()
    m.Initialize(cfg.pt_params(SEED), inst.m_hipscene, c.width, c.height, (0,) * n_dev)
    assert m.DeviceCount() == n_dev
    m.SetNoiseStats(True)
    poses = sequence(inst, case, sobol_matrices)
    for k in range(N_POSES):
        out = []
        for t in (single, m):
            go(t, cfg, poses[k])
            out.append(moments_call(t) + (t.ReadResult(),))
        assert same(out[0][4], out[1][4]), "the images differ"
        for i, name in enumerate(("result", "history length", "variance")):
            assert same(out[0][i], out[1][i]), "call at pose %d, %d shards against one context: %s" % (k, n_dev, name)
        assert out[0][3]["pixels_spatial"] == out[1][3]["pixels_spatial"] and out[1][3]["variance_ms"] > 0.0
    m.destroy()
    single.destroy()


def test_refusals(scene_cache, sobol_matrices):
    case = CASES[0]
    inst, _ = instance(scene_cache, case)
    p, cfg = inst.m_path_tracer, inst.m_config
    w, h = case[1:3]
    v = np.zeros((h, w), np.float32)

    def read_denoised():
        rgb = np.zeros((h, w, 3), F)
        p._call("read_denoised", rgb.ctypes.data)
        return rgb

    def nothing_left():
        return N.lib.adypt_read_denoise_variance(p._ctx, v.ctypes.data) == N.E_STATE and p.GetDenoiseMoments() == dict(have=0, variance_ms=0.0, pixels_spatial=0, device_bytes=0)
    pose = sequence(inst, case, sobol_matrices)[0]
    # read-outs before any moments call; 0 spp
    go(p, cfg, pose, 0)
    assert N.lib.adypt_read_denoise_variance(p._ctx, v.ctypes.data) == N.E_STATE and b"no moments call" in N.lib.adypt_last_error(p._ctx)
    assert nothing_left()
    with pytest.raises(N.AdyptError) as e:
        p.Denoise(temporal=True, moments=True)
    assert e.value.code == N.E_STATE and "not path-traced" in str(e.value), str(e.value)  # (nothing has been traced yet)
    assert nothing_left()
    p.Trace(True, 1)
    p.Reset()
    with pytest.raises(N.AdyptError) as e:
        p.Denoise(temporal=True, moments=True)
    assert e.value.code == N.E_STATE and "needs at least 1 spp in every block" in str(e.value), str(e.value)
    assert nothing_left()
    # 1 spp: every call but a moments call is refused with the message it always had
    p.Trace(True, 1)
    for kw in (dict(), dict(temporal=True), dict(temporal=True, follow_motion=True), dict(temporal=True, rectify=True)):
        with pytest.raises(N.AdyptError) as e:
            p.Denoise(**kw)
        assert e.value.code == N.E_STATE and "needs at least 2 spp in every block (the variance of a pixel's mean is not defined below)" in str(e.value), (kw, str(e.value))
    assert nothing_left()
    p.Trace(True, 1)
    last = p.Denoise(temporal=True)
    with pytest.raises(N.AdyptError) as e:
        p.ReadDenoiseVariance()
    assert e.value.code == N.E_STATE
    # what does not go with moments: refused before the library is asked
    for kw in (dict(moments=True), dict(temporal=True, moments=True, rectify=True), dict(temporal=True, moments=True, specular_bounces=2), dict(moments=True, specular_bounces=2)):
        with pytest.raises(ValueError):
            p.Denoise(**kw)
        assert same(read_denoised(), last) and nothing_left(), kw
    for kw, word in ((dict(history_cap=0.0), "history_cap"), (dict(history_cap=float("nan")), "history_cap"), (dict(levels=7), "levels must be in [1, 6]")):
        with pytest.raises(N.AdyptError) as e:
            p.Denoise(temporal=True, moments=True, **kw)
        assert e.value.code == N.E_INVALID and word in str(e.value), str(e.value)
        assert same(read_denoised(), last) and nothing_left(), "a refused call left something"
    # null pointers: the defaults (cap 64, committing)
    assert N.lib.adypt_denoise_temporal_moments(p._ctx, None, None, 0) == N.ADYPT_OK
    info = p.GetDenoiseMoments()
    assert info["have"] == 1 and info["device_bytes"] >= 4 * w * h + 512
    assert N.lib.adypt_read_denoise_variance(p._ctx, v.ctypes.data) == N.ADYPT_OK and np.isfinite(v).all() and (v >= 0).all()
    assert N.lib.adypt_read_denoise_variance(p._ctx, None) == N.E_INVALID and N.lib.adypt_get_denoise_moments(p._ctx, None) == N.E_INVALID
    p.Trace(False)
    with pytest.raises(N.AdyptError) as e:
        p.Denoise(temporal=True, moments=True)
    assert e.value.code == N.E_STATE and "not path-traced" in str(e.value)
    p.destroy()
    # a shard context
    part = TG.make_instance(scene_cache, "tiny0", 100, 75, rank=1, world=2)
    q = part.m_path_tracer
    q.SetNoiseStats(True)
    q.Trace(True, 1)
    with pytest.raises(N.AdyptError) as e:
        q.Denoise(temporal=True, moments=True)
    assert e.value.code == N.E_STATE and "tile shard" in str(e.value)
    q.destroy()


def test_cli(scene_cache, sobol_matrices, tmp_path):
    """--denoise-moments --spp 1 with two --history-from configs on sibenik 70x20 against the truth of the same sequence, the [PT]TEMPORAL: line and
    --variance-out; the same command line without the flag exits as it always did."""
    case = CASES[1]
    name, w, h = case[:3]
    inst, spec = instance(scene_cache, case)
    c, osc = inst.m_config.c, oracle_scene_from_instance(inst)
    main = json.load(open(spec.config_path))
    paths, hist = [], None
    for k in (1, 2):  # the earlier poses: two and one step away from the main config's camera, with the seeds the tool gives them
        pose = oracle_pose(case, osc, c, 3 - k, SEED + k, sobol_matrices)
        other = json.loads(json.dumps(main))
        other["camera"]["position"], other["camera"]["yaw"] = pose["pos"], pose["yaw"]
        paths.append(str(tmp_path / ("pose%d.config" % k)))
        json.dump(other, open(paths[-1], "w"), indent=4)
        _, _, hist, _ = MT.denoise(*pose["calls"][1], hist, pose["cam"])
    pose = oracle_pose(case, osc, c, 0, SEED, sobol_matrices)
    call = pose["calls"][1]
    den, length, _, extra = MT.denoise(*call, hist, pose["cam"])
    hit = call[6]
    inst.m_path_tracer.destroy()
    out, d_exr, l_exr, v_exr = (str(tmp_path / f) for f in ("o.exr", "d.exr", "l.exr", "v.exr"))
    copy = str(tmp_path / "main.config")  # (the tool writes its config back on exit)
    json.dump(main, open(copy, "w"), indent=4)

    def cli(*args):
        r = subprocess.run([CLI, copy, "--out", out, "--seed", str(SEED), "--spp", "1", "--denoise", d_exr, "--history-from", paths[0], "--history-from", paths[1]] + list(args),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        return r.returncode, (r.stdout + r.stderr).decode()
    code, text = cli()
    assert code == 2 and "--denoise needs --spp >= 2 and no --primary" in text and not os.path.exists(d_exr), text[-2000:]
    code, text = cli("--denoise-moments", "--history-out", l_exr, "--variance-out", v_exr)
    assert code == 0 and "Saved denoised image (5 levels)" in text, text[-2000:]
    assert same(api.load_exr(out), call[0]) and same(api.load_exr(d_exr), den), "the tool's images are not the truth's"
    assert same(api.load_exr(l_exr)[..., 0], length) and same(api.load_exr(v_exr)[..., 0], extra["V"])
    took = int((length[hit] > 1).sum())
    line = "[PT]TEMPORAL: history on %d of %d hit pixels, mean length %.3f, spatial variance on %d pixels\n" % (took, int(hit.sum()), float(length[hit].astype(np.float64).mean()),
                                                                                                              int(extra["spatial"].sum()))
    assert line in text and took > 0, text[-2000:]
