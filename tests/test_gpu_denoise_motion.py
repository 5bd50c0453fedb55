"""-m gpu: the temporal merge follows moved geometry (include/adypt_hip.h adypt_denoise_temporal_motion ...; temporal_previous_point and
temporal_merge_motion in csrc/device/temporal.hpp; k_motion_snapshot, k_motion_gather and k_temporal_merge<true> in denoise.hip).
The truth is computed in this process by the numpy restatement (tests/temporal_motion_truth.py) from what the CPU ORACLE gives for every pose — its
image, the moments of its samples, its primary frames, the triangle index and (u, v) of its primary hits — and from the host's vertex arrays of both
poses; never from the library's read-outs.  Everything is compared bit for bit.  tiny0 100x75, 4 spp, no sub-pixel jitter."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import temporal_motion_truth as TM  # noqa: E402
from tests import temporal_truth as TT  # noqa: E402
from tests import test_gpu_denoise as DN  # noqa: E402
from tests import test_gpu_noise as G  # noqa: E402
from tests.helpers import bits, oracle_scene_from_instance  # noqa: E402
from tests.test_gpu_denoise_temporal import GEOMETRY, MOVE, MOVED_BOX, SEED, SPP, camera_of, oracle_pose, same, set_pose  # noqa: E402
from tests.test_gpu_parity import make_instance  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "adypt_amd", "adypt_hip")
F = np.float32
ROTATION_DEGREES, ROTATION_MOVE = 40.0, (0.1, 0.2, 0.1)  # about the box's vertical axis; 0.2 upwards is past the plane tolerance (0.02 x 5.5) for its top too
_world = {}


def instance(scene_cache, w=GEOMETRY[1], h=GEOMETRY[2]):
    """tiny0 as tests/test_gpu_denoise_temporal.py's moving-geometry test makes it, its triangles and which of them are the box"""
    name, _, _, life, sub = GEOMETRY
    spec = scenes.make_scene(name, scene_cache, width=w, height=h, pt={"tmpLifetime": life, "maxBounce": 6, "subpixel": sub, "stackSize": 32})
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=SEED), api.InstanceConfig.last_error()
    inst.m_path_tracer.SetNoiseStats(True)
    tris = np.array(inst.scene.triangles).view(O.TRI_DT)
    lo, hi = np.array(MOVED_BOX[0]) - 1e-4, np.array(MOVED_BOX[1]) + 1e-4
    on_box = ((tris["p"] >= lo) & (tris["p"] <= hi)).all(axis=(1, 2))
    assert on_box.sum() == 12
    return inst, spec, tris, on_box


def words(tris):
    return TM.tri_words(tris["p"], tris["n"])


def rotation_matrices(tris, on_box):
    """(part of every triangle, [2, 3, 4]: the identity and the box's rotation about the vertical through its centre plus ROTATION_MOVE)"""
    centre = (np.array(MOVED_BOX[0]) + np.array(MOVED_BOX[1])) / 2
    t = np.radians(ROTATION_DEGREES)
    R = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
    m = np.zeros((2, 3, 4), np.float32)
    m[0, :, :3] = np.eye(3)
    m[1, :, :3], m[1, :, 3] = R, centre - R @ centre + np.array(ROTATION_MOVE)
    return on_box.astype(np.int32), m


def world(scene_cache, sobol_matrices):
    """Everything the oracle and numpy say about the poses of the cases below; once per session."""
    if _world:
        return _world
    inst, _, tris, on_box = instance(scene_cache)
    cfg, c = inst.m_config, inst.m_config.c

    def oracle_scene(t):
        b = api.WideBVH()
        b.BuildPLOC(api.Scene.FromArrays(t, inst.scene.materials), cfg.bvh_params(), 8, 0.0)
        return O.Scene(b.nodes, b.tri_indices, np.ascontiguousarray(t).view(np.uint8).reshape(-1), inst.scene.materials, textures=inst.scene.textures)

    def pose(key, osc, k, seed):
        pos, yaw = camera_of(c, GEOMETRY[0], k)
        call, cam, _, tri = oracle_pose(key, osc, c, pos, yaw, seed, sobol_matrices)
        ip, iv = O.camera(c.fov, yaw, c.pitch, c.width, c.height)
        P = O.make_params(c.width, c.height, pos, ip, iv, stack_size=c.stack_size, max_bounce=c.max_bounce, subpixel=c.subpixel, tmp_life=c.tmp_lifetime, tmin=c.ray_tmin,
                          clamp=c.clamp, sun=list(c.sun))
        hits = O.primary_frame(osc, P, 0)[1]
        assert np.array_equal(hits["tri_id"], tri)
        return dict(pos=pos, yaw=yaw, seed=seed, call=call, cam=cam, tri=tri, uv=np.stack([hits["u"], hits["v"]], -1).astype(np.float32))

    moved = tris.copy()
    moved["p"][on_box] += np.array(MOVE, np.float32)
    parts, matrices = rotation_matrices(tris, on_box)
    turned = np.array(api.pose_triangles(tris, matrices, parts=parts)).view(O.TRI_DT)
    without = np.ascontiguousarray(tris[~on_box])
    rest_scene = oracle_scene_from_instance(inst)
    w = _world
    w.update(tris=tris, on_box=on_box, box_ids=np.nonzero(on_box)[0], moved=moved, turned=turned, without=without, parts=parts, matrices=matrices)
    w["rest"] = pose(("geometry", "rest"), rest_scene, 0, SEED)  # (the first three keys: the poses of tests/test_gpu_denoise_temporal.py, computed once for both)
    w["box_moved"] = pose(("geometry", "moved"), oracle_scene(moved), 1, SEED + 1)
    w["box_removed"] = pose(("geometry", "removed"), oracle_scene(without), 1, SEED + 2)
    w["box_turned"] = pose(("geometry", "turned"), oracle_scene(turned), 1, SEED + 1)
    w["rest_later"] = pose(("geometry", "rest later"), rest_scene, 1, SEED + 1)
    r = w["rest"]
    _, _, w["hist"], _ = TM.denoise(*r["call"], None, r["cam"], r["tri"], r["uv"], words(tris))
    inst.m_path_tracer.destroy()
    return w


def truth(w, name, cur, hist=None, **kw):
    p = w[name]
    return TM.denoise(*p["call"], w["hist"] if hist is None else hist, p["cam"], p["tri"], p["uv"], words(cur), **kw)


def go(p, cfg, pose):
    set_pose(p, cfg, pose["pos"], pose["yaw"], pose["seed"])
    assert same(p.ReadResult(), pose["call"][0]), "the image is not the oracle's"
    assert np.array_equal(p.ReadHits()[0], pose["tri"])


def motion_call(p, **kw):
    """(result, history length, previous position, moved) of one Denoise(temporal=True, follow_motion=True)"""
    out = p.Denoise(temporal=True, follow_motion=True, **kw)
    m = p.ReadDenoiseMotion()
    return out, p.ReadDenoiseHistory(), m["previous_position"], m["moved"]


def assert_truth(got, want, tag):
    out, n_out, prev, moved = got
    w_out, w_n, _, w_motion = want
    assert same(out, w_out), tag + ": %d words of the result differ" % int((bits(out) != bits(w_out)).sum())
    assert same(n_out, w_n), tag + ": the history length"
    assert same(prev, w_motion["previous_position"]), tag + ": the previous position"
    assert np.array_equal(moved, w_motion["moved"]), tag + ": moved"


def commit_rest(p, cfg, w):
    go(p, cfg, w["rest"])
    got = motion_call(p)
    r = w["rest"]
    assert_truth(got, TM.denoise(*r["call"], None, r["cam"], r["tri"], r["uv"], words(w["tris"])), "the rest pose")
    assert not got[3].any()


def test_box_moved_and_the_camera_a_step_on(scene_cache, sobol_matrices):
    w = world(scene_cache, sobol_matrices)
    pose = w["box_moved"]
    want = truth(w, "box_moved", w["moved"])
    plain, plain_n, _ = TT.denoise(*pose["call"], w["hist"], pose["cam"])
    # the case, held on the CPU before the GPU is used: enough of the box in view, most of it finds its history, the rest keeps its own
    on_moved = np.isin(pose["tri"], w["box_ids"])
    static = (pose["tri"] >= 0) & ~on_moved
    took = want[1][on_moved] > F(SPP)
    print("box pixels %d, of them with history %d (%.3f); static pixels with history %.3f" % (on_moved.sum(), took.sum(), took.mean(), (want[1][static] > F(SPP)).mean()))
    assert on_moved.sum() > 50 and took.mean() > 0.5 and (want[1][static] > F(SPP)).mean() > 0.8
    assert (plain_n[on_moved] == F(SPP)).all()
    inst, _, _, _ = instance(scene_cache)
    p, cfg = inst.m_path_tracer, inst.m_config
    commit_rest(p, cfg, w)
    info = p.GetDenoiseMotion()
    assert info["have_snapshot"] == 1 and info["n_tris"] == len(w["tris"]) and info["device_bytes"] >= 80 * len(w["tris"]) + 32 * 100 * 75 and info["snapshot_ms"] > 0.0
    p.UpdateTriangles(0, w["moved"]["p"].reshape(-1, 9))
    go(p, cfg, pose)
    before = DN.state_of(p)
    got = motion_call(p, commit=False)
    assert_truth(got, want, "box moved")
    assert np.array_equal(got[3], on_moved), "moved is not exactly the pixels that hit one of the 12 box triangles"
    assert p.GetDenoiseMergeMs() > 0.0 and len(p.GetDenoiseTiming()["levels"]) == 5
    DN.assert_same_state(DN.state_of(p), before, "around the motion call")
    # without follow_motion: as before, the box starts again
    out, n_out = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
    assert same(out, plain) and same(n_out, plain_n) and (n_out[on_moved] == F(SPP)).all()
    # other filter parameters and a small cap
    kw = dict(levels=2, sigma_l=2.0, sigma_z=0.3)
    want2 = truth(w, "box_moved", w["moved"], cap=2.5, **kw)
    assert_truth(motion_call(p, history_cap=2.5, commit=False, **kw), want2, "cap 2.5, 2 levels")
    p.destroy()


def test_rotation_through_bind_parts_and_pose(scene_cache, sobol_matrices):
    w = world(scene_cache, sobol_matrices)
    pose = w["box_turned"]
    want = truth(w, "box_turned", w["turned"])
    _, plain_n, _ = TT.denoise(*pose["call"], w["hist"], pose["cam"])
    on_moved = np.isin(pose["tri"], w["box_ids"])
    took = want[1][on_moved] > F(SPP)
    print("turned box pixels %d, of them with history %d (%.3f)" % (on_moved.sum(), took.sum(), took.mean()))
    assert on_moved.sum() > 50 and (plain_n[on_moved] == F(SPP)).all(), "the plain call does not refuse the turned box"
    assert took.sum() > 50, "the motion call finds next to nothing on the turned box"
    inst, _, _, _ = instance(scene_cache)
    p, cfg = inst.m_path_tracer, inst.m_config
    commit_rest(p, cfg, w)
    p.BindParts(w["parts"], 2)
    p.Pose(w["matrices"])
    assert same(np.array(p.ReadTriangles()).view(O.TRI_DT)["p"], w["turned"]["p"])
    go(p, cfg, pose)
    got = motion_call(p, commit=False)
    assert_truth(got, want, "box turned")
    out, n_out = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
    assert same(n_out, plain_n)
    # a new tree keeps every triangle's index: the snapshot survives it
    p.RebuildBVH(method="ploc")
    assert p.GetDenoiseMotion()["have_snapshot"] == 1
    go(p, cfg, pose)
    assert_truth(motion_call(p, commit=False), want, "after RebuildBVH(method='ploc')")
    p.destroy()


def test_nothing_moved_is_the_plain_call(scene_cache, sobol_matrices):
    w = world(scene_cache, sobol_matrices)
    pose = w["rest_later"]
    inst, _, _, _ = instance(scene_cache)
    p, cfg = inst.m_path_tracer, inst.m_config
    commit_rest(p, cfg, w)
    go(p, cfg, pose)
    want, want_n, _ = TT.denoise(*pose["call"], w["hist"], pose["cam"])
    plain, plain_n = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
    got = motion_call(p, commit=False)
    assert same(plain, want) and same(plain_n, want_n)
    assert same(got[0], plain) and same(got[1], plain_n) and not got[3].any() and same(got[2], pose["call"][5])
    assert (want_n[pose["call"][6]] > F(SPP)).mean() > 0.8
    p.destroy()


def test_snapshot_lifetime(scene_cache, sobol_matrices):
    w = world(scene_cache, sobol_matrices)
    inst, _, _, _ = instance(scene_cache)
    p, cfg = inst.m_path_tracer, inst.m_config
    have = lambda: p.GetDenoiseMotion()["have_snapshot"]  # noqa: E731
    assert have() == 0 and p.GetDenoiseMotion()["n_tris"] == 0
    commit_rest(p, cfg, w)
    assert have() == 1
    # commit=False leaves it
    p.UpdateTriangles(0, w["moved"]["p"].reshape(-1, 9))
    go(p, cfg, w["box_moved"])
    want = truth(w, "box_moved", w["moved"])
    for k in range(2):
        assert_truth(motion_call(p, commit=False), want, "commit=False, call %d" % k)
    assert have() == 1
    # SetTriangles drops it (an index means another triangle): the call is the plain call, which tests/test_gpu_denoise_temporal.py holds against numpy
    pose = w["box_removed"]
    p.SetTriangles(w["without"].view(np.uint8).reshape(-1))
    assert have() == 0
    go(p, cfg, pose)
    want2, want_n2, _ = TT.denoise(*pose["call"], w["hist"], pose["cam"])
    got = motion_call(p, commit=False)
    assert same(got[0], want2) and same(got[1], want_n2) and not got[3].any()
    # a committing motion call makes one of the new triangles; a committing call without motion drops it: the history's geometry is unknown
    motion_call(p)
    info = p.GetDenoiseMotion()
    assert info["have_snapshot"] == 1 and info["n_tris"] == len(w["without"])
    p.Denoise(temporal=True)
    assert have() == 0
    plain, plain_n = p.Denoise(temporal=True, commit=False), p.ReadDenoiseHistory()
    got = motion_call(p, commit=False)
    assert same(got[0], plain) and same(got[1], plain_n) and not got[3].any() and (plain_n > F(SPP)).mean() > 0.5
    # ResetDenoiseHistory() drops it with the history
    motion_call(p)
    assert have() == 1
    p.ResetDenoiseHistory()
    assert have() == 0
    got = motion_call(p, commit=False)
    assert same(got[0], p.Denoise()) and (got[1] == F(SPP)).all() and not got[3].any()
    p.destroy()


@pytest.mark.parametrize("shape,n_dev", [((100, 75), 2), ((100, 75), 3), ((64, 36), 4)], ids=["100x75-2", "100x75-3", "64x36-4-one-owns-nothing"])
def test_several_shards_on_one_card(shape, n_dev, scene_cache, monkeypatch):
    """Several shards on one card against one context over two committing motion calls with the box moved in between: identical bits (the
    one-context bits are held against numpy above)."""
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    inst, _, tris, on_box = instance(scene_cache, *shape)
    single, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    m = api.MultiPathTracer()
    m.Initialize(cfg.pt_params(SEED), inst.m_hipscene, c.width, c.height, (0,) * n_dev)
    assert m.DeviceCount() == n_dev
    if shape == (64, 36):
        assert any(N.lib.adypt_local_pixel_count(x) == 0 for x in m._contexts())
    m.SetNoiseStats(True)
    moved = tris.copy()
    moved["p"][on_box] += np.array(MOVE, np.float32)
    for k in range(2):
        pos, yaw = camera_of(c, GEOMETRY[0], k)
        out = []
        for t in (single, m):
            if k == 1:
                t.UpdateTriangles(0, moved["p"].reshape(-1, 9))
            set_pose(t, cfg, pos, yaw, SEED + k)
            out.append((t.ReadResult(),) + motion_call(t))
        for i, what in enumerate(("the image", "the result", "the history length", "the previous position", "moved")):
            assert same(np.asarray(out[0][i], np.float32), np.asarray(out[1][i], np.float32)), "call %d, %d shards against one context: %s" % (k, n_dev, what)
    assert out[1][4].any() and (out[1][2][out[1][4]] > F(SPP)).any(), "no moved pixel found history"
    assert m.GetDenoiseMotion() == dict(single.GetDenoiseMotion(), snapshot_ms=m.GetDenoiseMotion()["snapshot_ms"]) and m.GetDenoiseMergeMs() > 0.0
    # a shard context refuses the per-context call
    with pytest.raises(N.AdyptError) as e:
        N.check(N.lib.adypt_denoise_temporal_motion(m._contexts()[0], None, None), m._contexts()[0])
    assert e.value.code == N.E_STATE and "tile shard" in str(e.value)
    m.destroy()
    single.destroy()


def test_refusals(scene_cache):
    inst = make_instance(scene_cache, "tiny0", 96, 64)
    p = inst.m_path_tracer
    prev, moved = np.zeros((64, 96, 3), np.float32), np.zeros((64, 96), np.uint8)
    with pytest.raises(ValueError):
        p.Denoise(follow_motion=True)
    assert N.lib.adypt_read_denoise_motion(p._ctx, prev.ctypes.data, moved.ctypes.data) == N.E_STATE and b"no motion call" in N.lib.adypt_last_error(p._ctx)
    assert p.GetDenoiseMotion() == {"have_snapshot": 0, "snapshot_ms": 0.0, "n_tris": 0, "device_bytes": 0}

    def refused(code, word, **kw):
        with pytest.raises(N.AdyptError) as e:
            p.Denoise(temporal=True, follow_motion=True, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)
    p.Trace(True, 4)
    refused(N.E_STATE, "statistics are off")
    p.Reset()
    p.SetNoiseStats(True)
    p.Trace(True, 1)
    refused(N.E_STATE, "at least 2 spp")
    p.Trace(True, 1)
    for bad in (0.0, float("nan"), float("inf")):
        refused(N.E_INVALID, "history_cap must be a positive finite number", history_cap=bad)
    refused(N.E_INVALID, "levels must be in [1, 6]", levels=7)
    p.Denoise(temporal=True)
    assert N.lib.adypt_read_denoise_motion(p._ctx, prev.ctypes.data, moved.ctypes.data) == N.E_STATE  # a temporal call without motion leaves nothing to read
    assert N.lib.adypt_denoise_temporal_motion(p._ctx, None, None) == N.ADYPT_OK  # null pointers: the defaults (cap 64, committing)
    assert N.lib.adypt_read_denoise_motion(p._ctx, None, moved.ctypes.data) == N.ADYPT_OK and not moved.any()
    assert N.lib.adypt_read_denoise_motion(p._ctx, prev.ctypes.data, None) == N.ADYPT_OK and same(prev, p.ReadDenoiseGuides()["position"])
    assert N.lib.adypt_get_denoise_motion(p._ctx, None) == N.E_INVALID
    p.destroy()


def test_cli_follows_the_parts_it_moves(scene_cache, tmp_path):
    """--follow-motion with two --history-from configs and --part-matrices on tiny0 96x64 against the same sequence through Python: the history poses
    see the scene as loaded, then the box's part is moved and the main config rendered."""
    case = G.CASES[1]
    name, w, h = case[:3]
    inst, spec = G._instance(scene_cache, case)
    p, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    p.SetNoiseStats(True)
    tris = np.array(inst.scene.triangles).view(O.TRI_DT)
    lo, hi = np.array(MOVED_BOX[0]) - 1e-4, np.array(MOVED_BOX[1]) + 1e-4
    on_box = ((tris["p"] >= lo) & (tris["p"] <= hi)).all(axis=(1, 2))
    n_mats = len(np.asarray(inst.scene.materials).view(np.uint8).reshape(-1)) // 64
    box_part = np.unique(tris["matid"][on_box])
    assert len(box_part) == 1 and 0 <= box_part[0] < n_mats
    known = (tris["matid"] >= 0) & (tris["matid"] < n_mats)
    parts, n_parts = np.where(known, tris["matid"], n_mats).astype(np.int32), n_mats + (0 if known.all() else 1)
    matrices = np.zeros((n_parts, 3, 4), np.float32)
    matrices[:, :, :3] = np.eye(3)
    matrices[box_part[0], :, 3] = MOVE
    matrix_file = str(tmp_path / "parts.txt")
    open(matrix_file, "w").write("# the box\n%d %s\n" % (box_part[0], " ".join(repr(float(v)) for v in matrices[box_part[0]].reshape(-1))))
    main = json.load(open(spec.config_path))
    paths = []
    for k in (1, 2):
        pos, yaw = camera_of(c, name, 3 - k)
        other = json.loads(json.dumps(main))
        other["camera"]["position"], other["camera"]["yaw"] = pos, yaw
        paths.append(str(tmp_path / ("pose%d.config" % k)))
        json.dump(other, open(paths[-1], "w"), indent=4)
        set_pose(p, cfg, pos, yaw, SEED + k)
        p.Denoise(temporal=True, history_cap=16.0, follow_motion=True)
    p.BindParts(parts, n_parts)
    p.Pose(matrices)
    pos, yaw = camera_of(c, name, 0)
    set_pose(p, cfg, pos, yaw, SEED)
    img, den, length = p.ReadResult(), p.Denoise(temporal=True, history_cap=16.0, follow_motion=True), p.ReadDenoiseHistory()
    hit, moved = p.ReadDenoiseGuides()["hit"], p.ReadDenoiseMotion()["moved"]
    p.destroy()
    assert moved.sum() > 20 and (length[moved] > SPP).mean() > 0.5, "the case shows next to nothing of the moved box"
    out, d_exr, l_exr = str(tmp_path / "o.exr"), str(tmp_path / "d.exr"), str(tmp_path / "l.exr")
    copy = str(tmp_path / "main.config")  # (the tool writes its config back on exit)
    json.dump(main, open(copy, "w"), indent=4)

    def cli(*args):
        r = subprocess.run([CLI, copy, "--out", out, "--seed", str(SEED), "--spp", str(SPP)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        return r.returncode, (r.stdout + r.stderr).decode()
    history = ["--history-from", paths[0], "--history-from", paths[1], "--history-cap", "16", "--history-out", l_exr]
    code, text = cli("--denoise", d_exr, "--part-matrices", matrix_file, "--follow-motion", *history)
    assert code == 0 and "Saved denoised image (5 levels)" in text, text[-2000:]
    assert same(api.load_exr(out), img) and same(api.load_exr(d_exr), den), "the tool's images are not the Python sequence's"
    assert same(api.load_exr(l_exr)[..., 0], length)
    took = int((length[hit] > SPP).sum())
    line = "[PT]TEMPORAL: history on %d of %d hit pixels, mean length %.3f, moved %d pixels\n" % (took, int(hit.sum()), float(length[hit].astype(np.float64).mean()), int(moved.sum()))
    assert line in text, text[-2000:]
    assert text.index("history pose") < text.index("[PT]POSE:"), "the pose was applied before the history poses"
    # without the flag the pose comes first and the line is the old one
    code, text = cli("--denoise", d_exr, "--part-matrices", matrix_file, *history)
    assert code == 0 and text.index("[PT]POSE:") < text.index("history pose") and "moved" not in text.split("[PT]TEMPORAL:")[1].splitlines()[0], text[-2000:]
    # (the flag needs a temporal call: tests/test_cli_options.py)
