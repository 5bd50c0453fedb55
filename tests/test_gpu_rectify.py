"""-m gpu: rectifying stale history (include/adypt_hip.h adypt_denoise_temporal_rectified ...; csrc/device/rectify.hpp, k_rectify_window and
k_temporal_merge<., true> in denoise.hip).  The truth is computed in this process by the numpy restatement of the definition (tests/rectify_truth.py)
from what the CPU ORACLE gives for every pose — its image, the moments of its exact per-frame samples, its primary frames of types 0 / 4 / 5 — never
from the library's read-outs; the history of the truth is the truth's own.  Three poses a camera step apart, the last under a quarter of the config's
sun (the light changes on surfaces that stand still).  Everything is compared bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import noise_truth as T  # noqa: E402
from tests import rectify_truth as RT  # noqa: E402
from tests import temporal_truth as TT  # noqa: E402
from tests import test_gpu_denoise as DN  # noqa: E402          (its state snapshots)
from tests import test_gpu_denoise_motion as M  # noqa: E402   (its moved box and what the oracle says about it)
from tests import test_gpu_denoise_temporal as TG  # noqa: E402 (its camera steps)
from tests.helpers import bits, oracle_scene_from_instance  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "adypt_amd", "adypt_hip")
SEED, SPP = TG.SEED, TG.SPP
F = np.float32
DIM = 0.25  # the sun of the last pose, as a share of the config's
#        scene      w    h  life sub
CASES = [("tiny0", 33, 9, 16, 3),      # one pixel past a workgroup (32 x 8) in x and in y: a tile's halo clips on all four sides of the image
         ("tiny0", 100, 75, 16, 3),    # partial workgroups and partial blocks on two edges
         ("sibenik", 160, 90, 3, 1)]
IDS = ["%s-%dx%d" % c[:3] for c in CASES]
same = TG.same
_poses = {}


def instance(scene_cache, case):
    name, w, h, life, sub = case
    spec = scenes.make_scene(name, scene_cache, width=w, height=h, pt={"tmpLifetime": life, "maxBounce": 6, "subpixel": sub})
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=SEED), api.InstanceConfig.last_error()
    inst.m_path_tracer.SetNoiseStats(True)
    return inst, spec


def sun_of(c, scale):
    return [float(F(v) * F(scale)) for v in c.sun]


def oracle_pose(key, osc, c, k, seed, scale, sobol_matrices, frames=SPP + 2):
    """What the oracle gives for the case's camera k steps on under the sun times `scale`: dict(pos, yaw, seed, scale, call (the filter's inputs after SPP
    frames), cam, images (after every frame), tri); once per key."""
    key = key + (k, seed, scale)
    if key not in _poses:
        pos, yaw = TG.camera_of(c, key[0], k)
        w, h = c.width, c.height
        ip, iv = O.camera(c.fov, yaw, c.pitch, w, h)
        P = O.make_params(w, h, pos, ip, iv, stack_size=c.stack_size, max_bounce=c.max_bounce, subpixel=c.subpixel, tmp_life=c.tmp_lifetime, tmin=c.ray_tmin,
                          clamp=c.clamp, sun=sun_of(c, scale))
        shift = O.shift_bytes(seed, w, h)
        _, m2 = T.moments(T.frame_samples(osc, P, shift, sobol_matrices, SPP))
        state, images = O.PathTracerState(w, h), []
        for _ in range(frames):
            O.pt_frames(osc, P, shift, sobol_matrices, state, 1)
            images.append(state.accum[..., :3].copy())
        g = [O.primary_frame(osc, P, t) for t in (0, 4, 5)]
        tri = g[0][1]["tri_id"].copy()
        call = (images[SPP - 1], m2, SPP, g[0][0][..., :3].copy(), g[1][0][..., :3].copy(), g[2][0][..., :3].copy(), tri != -1)
        _poses[key] = dict(pos=pos, yaw=yaw, seed=seed, scale=scale, call=call, cam=(np.array(pos, np.float32), ip, iv), images=images, tri=tri)
    return _poses[key]


def sequence(inst, case, sobol_matrices, n=3):
    """the oracle's poses of the case's first n cameras, each with a seed of its own, the last under the dimmed sun"""
    c, osc = inst.m_config.c, oracle_scene_from_instance(inst)
    return [oracle_pose(case, osc, c, k, SEED + k, DIM if k == n - 1 else 1.0, sobol_matrices) for k in range(n)]


def go(t, cfg, pose, spp=SPP):
    """the tracer at 0 spp under the pose's camera, seed and sun, then spp frames"""
    c = cfg.c
    t.Reset()
    prm = cfg.pt_params(pose["seed"])
    prm.sun[:] = sun_of(c, pose["scale"])
    t.SetConfig(prm)
    ip, iv = api.camera_matrices(c.fov, pose["yaw"], c.pitch, c.width, c.height)
    t.SetCamera(ip, iv, np.array(pose["pos"], np.float32))
    if spp:
        t.Trace(True, spp)


def rectified(t, **kw):
    """(result, history length, kept) of one rectified call"""
    return t.Denoise(temporal=True, rectify=True, **kw), t.ReadDenoiseHistory(), t.ReadDenoiseRectify()


def assert_truth(got, want, tag):
    out, n_out, kept = got
    w_out, w_n, _, extra = want
    assert same(out, w_out), "%s: %d words of the result differ" % (tag, int((bits(out) != bits(w_out)).sum()))
    assert same(n_out, w_n), "%s: %d words of the history length differ" % (tag, int((bits(n_out) != bits(w_n)).sum()))
    assert same(kept, extra["kept"]), "%s: %d words of kept differ" % (tag, int((bits(kept) != bits(extra["kept"])).sum()))


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_three_poses_the_last_under_a_dimmed_sun(case, radius, scene_cache, sobol_matrices):
    inst, _ = instance(scene_cache, case)
    p, cfg = inst.m_path_tracer, inst.m_config
    w, h = case[1:3]
    hist = None
    for k, pose in enumerate(sequence(inst, case, sobol_matrices)):
        go(p, cfg, pose)
        assert same(p.ReadResult(), pose["images"][SPP - 1]), "pose %d: the image is not the oracle's" % k
        before, hits_before = DN.state_of(p), p.ReadHits()
        want = RT.denoise(*pose["call"], hist, pose["cam"], radius=radius)
        if k == 1:
            # the history is only read: two calls give the same bits, and the committing call after them what it would have given without them
            assert_truth(rectified(p, rectify_radius=radius, commit=False), want, "commit=False")
            assert_truth(rectified(p, rectify_radius=radius, commit=False), want, "commit=False, again")
        assert_truth(rectified(p, rectify_radius=radius), want, "pose %d" % k)
        info = p.GetDenoiseRectify()
        assert info["have"] == 1 and info["radius"] == radius and info["gamma"] == 1.0 and info["window_ms"] > 0.0 and info["device_bytes"] >= 36 * w * h, info
        assert p.GetDenoiseMergeMs() >= info["window_ms"] and len(p.GetDenoiseTiming()["levels"]) == 5
        DN.assert_same_state(DN.state_of(p), before, "around the rectified call at pose %d" % k)
        hits_after = p.ReadHits()
        assert np.array_equal(hits_after[0], hits_before[0]) and same(hits_after[1], hits_before[1]), "the primary-hit cache moved"
        hist = want[2]
    hit, kept = pose["call"][6], want[3]["kept"]
    share = float((kept[hit] < 1).mean())
    print("%s radius %d: kept < 1 on %.1f %% of the %d hit pixels of the last pose, mean kept %.3f" % (IDS[CASES.index(case)], radius, 100.0 * share, int(hit.sum()), float(kept[hit].mean())))
    assert share > 0.0, "the case rectifies nothing: it shows nothing"
    p.Trace(True, 2)
    assert p.GetSPP() == SPP + 2 and same(p.ReadResult(), pose["images"][SPP + 1]), "tracing on after the rectified calls left the oracle's image"
    p.destroy()


def test_plain_temporal_calls_around_a_rectified_one_and_other_parameters(scene_cache, sobol_matrices):
    case = CASES[1]
    inst, _ = instance(scene_cache, case)
    p, cfg = inst.m_path_tracer, inst.m_config
    poses = sequence(inst, case, sobol_matrices)
    go(p, cfg, poses[0])
    p.Denoise(temporal=True)
    _, _, hist = TT.denoise(*poses[0]["call"], None, poses[0]["cam"])
    pose = poses[2]  # (the dimmed one, straight after the first: two camera steps)
    go(p, cfg, pose)
    want, want_n, _ = TT.denoise(*pose["call"], hist, pose["cam"])
    a, na = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
    assert same(a, want) and same(na, want_n)
    truth = RT.denoise(*pose["call"], hist, pose["cam"])
    got = rectified(p, commit=False)
    assert_truth(got, truth, "rectified between two plain calls")
    assert not same(got[0], a)
    b, nb = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
    assert same(b, want) and same(nb, want_n), "a plain temporal call after a rectified one is not what it was before it"
    assert same(p.ReadDenoiseRectify(), truth[3]["kept"]), "a plain temporal call moved the kept read-out"
    plain = p.Denoise()
    assert same(plain, DN.D.denoise(*pose["call"])) and same(p.ReadDenoiseRectify(), truth[3]["kept"])
    # other parameters: gamma 0 drops every history that is not its window's mean, a wide gamma keeps every one; a cap, two levels
    got, none = rectified(p, rectify_gamma=0.0, commit=False), RT.denoise(*pose["call"], hist, pose["cam"], gamma=0.0)
    assert_truth(got, none, "gamma 0")
    judged = none[3]["R0"][..., 3] >= F(4)  # (the pixels whose window says anything)
    assert judged.sum() > 1000 and (got[1][judged] == F(SPP)).all() and (want_n[judged] > F(SPP)).mean() > 0.5, "gamma 0 left a history standing"
    got = rectified(p, rectify_gamma=1.0e6, commit=False)
    assert_truth(got, RT.denoise(*pose["call"], hist, pose["cam"], gamma=1.0e6), "gamma 1e6")
    assert (got[2] == F(1)).all() and same(got[0], want) and same(got[1], want_n)
    kw = dict(levels=2, sigma_l=2.0, sigma_z=0.3)
    got = rectified(p, rectify_gamma=2.0, rectify_radius=2, history_cap=2.5, commit=False, **kw)
    assert_truth(got, RT.denoise(*pose["call"], hist, pose["cam"], radius=2, gamma=2.0, cap=2.5, **kw), "gamma 2, radius 2, cap 2.5, 2 levels")
    assert p.GetDenoiseRectify()["radius"] == 2 and p.GetDenoiseRectify()["gamma"] == 2.0
    p.destroy()


def test_rectified_and_following_moved_geometry(scene_cache, sobol_matrices):
    """tests/test_gpu_denoise_motion.py's box, moved between the committed pose and the measured one: the history is found through the previous pose and
    rectified against the current one's window."""
    w = M.world(scene_cache, sobol_matrices)
    pose = w["box_moved"]
    want = RT.denoise(*pose["call"], w["hist"], pose["cam"], motion=(pose["tri"], pose["uv"], M.words(w["moved"])))
    on_moved = np.isin(pose["tri"], w["box_ids"])
    assert (want[1][on_moved] > F(SPP)).mean() > 0.3 and (want[3]["kept"] < 1).any(), "the case: box pixels with history, and pixels with a rectified one"
    inst, _, _, _ = M.instance(scene_cache)
    p, cfg = inst.m_path_tracer, inst.m_config
    M.commit_rest(p, cfg, w)
    p.UpdateTriangles(0, w["moved"]["p"].reshape(-1, 9))
    M.go(p, cfg, pose)
    got = rectified(p, follow_motion=True, commit=False)
    assert_truth(got, want, "box moved, rectified")
    motion = p.ReadDenoiseMotion()
    assert np.array_equal(motion["moved"], on_moved)
    # without follow_motion the box starts again, rectified or not
    got = rectified(p, commit=False)
    assert_truth(got, RT.denoise(*pose["call"], w["hist"], pose["cam"]), "box moved, rectified, not followed")
    assert (got[1][on_moved] == F(SPP)).all() and (got[2][on_moved] == F(1)).all()
    # a committing rectified motion call keeps the snapshot: the next one still follows
    assert_truth(rectified(p, follow_motion=True), want, "committing")
    assert p.GetDenoiseMotion()["have_snapshot"] == 1
    p.destroy()


@pytest.mark.parametrize("n_dev", [2, 3])
def test_multi_device_on_one_card(n_dev, scene_cache, sobol_matrices, monkeypatch):
    """Several shards on one card against one context over two committing rectified calls: identical bits (the one-context bits are held against numpy above)."""
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = CASES[1]
    inst, _ = instance(scene_cache, case)
    single, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    m = api.MultiPathTracer()
    m.Initialize(cfg.pt_params(SEED), inst.m_hipscene, c.width, c.height, (0,) * n_dev)
    assert m.DeviceCount() == n_dev
    m.SetNoiseStats(True)
    poses = sequence(inst, case, sobol_matrices)
    for k in (0, 2):
        out = []
        for t in (single, m):
            go(t, cfg, poses[k])
            out.append(rectified(t) + (t.ReadResult(),))
        assert same(out[0][3], out[1][3]), "the images differ"
        for i, name in enumerate(("result", "history length", "kept")):
            assert same(out[0][i], out[1][i]), "call at pose %d, %d shards against one context: %s" % (k, n_dev, name)
    assert (out[1][2] < 1).any() and m.GetDenoiseRectify()["window_ms"] > 0.0 and m.GetDenoiseRectify()["radius"] == 3
    m.destroy()
    single.destroy()


def test_refusals(scene_cache, sobol_matrices):
    case = CASES[0]
    inst, _ = instance(scene_cache, case)
    p, cfg = inst.m_path_tracer, inst.m_config
    w, h = case[1:3]
    kept = np.zeros((h, w), np.float32)

    def read_denoised():
        rgb = np.zeros((h, w, 3), F)
        p._call("read_denoised", rgb.ctypes.data)
        return rgb
    go(p, cfg, sequence(inst, case, sobol_matrices)[0])
    # read-outs before any rectified call
    assert N.lib.adypt_read_denoise_rectify(p._ctx, kept.ctypes.data) == N.E_STATE and b"no rectified call" in N.lib.adypt_last_error(p._ctx)
    assert p.GetDenoiseRectify() == dict(have=0, radius=0, gamma=0.0, window_ms=0.0, device_bytes=0)
    last = p.Denoise(temporal=True)
    with pytest.raises(N.AdyptError) as e:
        p.ReadDenoiseRectify()
    assert e.value.code == N.E_STATE
    for kw in (dict(rectify_radius=0), dict(rectify_radius=4), dict(rectify_gamma=-1.0), dict(rectify_gamma=float("nan")), dict(rectify_gamma=float("inf"))):
        with pytest.raises(N.AdyptError) as e:
            p.Denoise(temporal=True, rectify=True, **kw)
        assert e.value.code == N.E_INVALID and "rectify radius must be in [1, 3]" in str(e.value), str(e.value)
        assert same(read_denoised(), last), "a refused call moved the last result"
        assert N.lib.adypt_read_denoise_rectify(p._ctx, kept.ctypes.data) == N.E_STATE and p.GetDenoiseRectify()["device_bytes"] == 0, "a refused call left something"
    with pytest.raises(ValueError):
        p.Denoise(rectify=True)
    assert same(read_denoised(), last)
    with pytest.raises(N.AdyptError) as e:
        p.Denoise(temporal=True, rectify=True, history_cap=0.0)
    assert e.value.code == N.E_INVALID and "history_cap" in str(e.value)
    # null pointers: the defaults (radius 3, gamma 1), on its own history under an unchanged camera
    assert N.lib.adypt_denoise_temporal_rectified(p._ctx, None, None, None, 0) == N.ADYPT_OK
    info = p.GetDenoiseRectify()
    assert info["have"] == 1 and info["radius"] == 3 and info["gamma"] == 1.0 and info["device_bytes"] >= 36 * w * h
    assert N.lib.adypt_read_denoise_rectify(p._ctx, kept.ctypes.data) == N.ADYPT_OK and (kept >= 0).all() and (kept <= 1).all()
    assert N.lib.adypt_read_denoise_rectify(p._ctx, None) == N.E_INVALID and N.lib.adypt_get_denoise_rectify(p._ctx, None) == N.E_INVALID
    p.destroy()


def test_cli(scene_cache, sobol_matrices, tmp_path):
    """Two --history-from configs on tiny0 100x75 with --rectify against the truth of the same sequence, and the [PT]TEMPORAL: line against kept."""
    case = CASES[1]
    name, w, h = case[:3]
    inst, spec = instance(scene_cache, case)
    c, osc = inst.m_config.c, oracle_scene_from_instance(inst)
    main = json.load(open(spec.config_path))
    paths, hist = [], None
    for k in (1, 2):  # the earlier poses: two and one step away from the main config's camera, with the seeds the tool gives them
        pose = oracle_pose(case, osc, c, 3 - k, SEED + k, 1.0, sobol_matrices, frames=SPP)
        other = json.loads(json.dumps(main))
        other["camera"]["position"], other["camera"]["yaw"] = pose["pos"], pose["yaw"]
        paths.append(str(tmp_path / ("pose%d.config" % k)))
        json.dump(other, open(paths[-1], "w"), indent=4)
        _, _, hist, _ = RT.denoise(*pose["call"], hist, pose["cam"], radius=2, gamma=1.5, cap=16.0)
    pose = oracle_pose(case, osc, c, 0, SEED, 1.0, sobol_matrices, frames=SPP)
    den, length, _, extra = RT.denoise(*pose["call"], hist, pose["cam"], radius=2, gamma=1.5, cap=16.0)
    hit, kept = pose["call"][6], extra["kept"]
    inst.m_path_tracer.destroy()
    out, d_exr, l_exr, k_exr = (str(tmp_path / f) for f in ("o.exr", "d.exr", "l.exr", "k.exr"))
    copy = str(tmp_path / "main.config")  # (the tool writes its config back on exit)
    json.dump(main, open(copy, "w"), indent=4)

    def cli(*args):
        r = subprocess.run([CLI, copy, "--out", out, "--seed", str(SEED), "--spp", str(SPP)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        return r.returncode, (r.stdout + r.stderr).decode()
    code, text = cli("--denoise", d_exr, "--history-from", paths[0], "--history-from", paths[1], "--history-cap", "16", "--history-out", l_exr, "--rectify", "--rectify-gamma", "1.5",
                     "--rectify-radius", "2", "--rectify-out", k_exr)
    assert code == 0 and "Saved denoised image (5 levels)" in text, text[-2000:]
    assert same(api.load_exr(out), pose["call"][0]) and same(api.load_exr(d_exr), den), "the tool's images are not the truth's"
    assert same(api.load_exr(l_exr)[..., 0], length) and same(api.load_exr(k_exr)[..., 0], kept)
    took = int((length[hit] > SPP).sum())
    line = "[PT]TEMPORAL: history on %d of %d hit pixels, mean length %.3f, rectified %d pixels\n" % (took, int(hit.sum()), float(length[hit].astype(np.float64).mean()), int((kept < 1).sum()))
    assert line in text, text[-2000:]
    assert (kept < 1).sum() > 0
    # (what the command line refuses of these options: tests/test_cli_options.py)
