"""Parity tests proper (-m gpu): the HIP path, called through the C-ABI, against the CPU oracle on the same seeded
inputs and against the committed golden vectors.  Bar: bit-exact — triangle ids, node-visit hashes, u/v/t bit
patterns, and (thanks to the pinned canonical arithmetic) every accumulated radiance pixel."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, distributed as D, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests.helpers import (GOLDEN, bits, golden_scene, oracle_params_from_config, oracle_scene_from_instance,  # noqa: E402
                           random_rays)


def make_instance(cache, name, w, h, pt=None, seed=99, rank=0, world=1, camera=None):
    spec = scenes.make_scene(name, cache, width=w, height=h, pt=pt, camera=camera)
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=seed, tile_rank=rank, tile_nranks=world), api.InstanceConfig.last_error()
    return inst


def golden_tracer(name, w=64, h=36, stack=32):
    _, idx, nodes, tris, mats, woop = golden_scene(name)
    sc = api.Scene.FromArrays(tris, mats)
    b = api.WideBVH()
    b.nodes, b.tri_indices = nodes.view("u1").reshape(-1), idx
    hs = api.HipScene()
    hs.Initialize(sc, b, woop=woop)  # the reference's own node / index / Woop arrays go straight into HBM
    cfg = api.InstanceConfig()
    p = cfg.pt_params(0)
    p.stack_size = stack
    pt = api.HipPathTracer()
    pt.Initialize(p, hs, w, h)
    return pt


@pytest.mark.parametrize("name", ["tiny0", "tiny1", "tiny2"])
def test_golden_known_answers_on_reference_built_arrays(name):
    """G5 through the HIP kernel, fed with the arrays the REFERENCE builder and init_triangles produced."""
    kat = np.load(os.path.join(GOLDEN, name + "_kat.npz"))
    pt = golden_tracer(name)
    hits = pt.TraceRays(kat["rays"], with_stats=True)
    assert hits.tobytes() == kat["hits"].tobytes()
    fov, yaw, pitch, px, py, pz = kat["cam"]
    ip, iv = api.camera_matrices(float(fov), float(yaw), float(pitch), 64, 36)
    pt.SetCamera(ip, iv, [px, py, pz])
    pt.Trace(False)
    tri, uv = pt.ReadHits()
    ph = kat["primary_hits"]
    assert np.array_equal(tri, ph["tri_id"])
    m = ph["tri_id"] >= 0
    assert np.array_equal(bits(uv[..., 0])[m], bits(ph["u"])[m]) and np.array_equal(bits(uv[..., 1])[m], bits(ph["v"])[m])
    assert np.array_equal(bits(pt.ReadResult()), bits(kat["primary_rgba"][..., :3]))


def test_golden_end_to_end_frame(sobol_matrices):
    """G6: 32x18, 4 spp with subpixel 2 / tmpLife 2 (primary-hit cache + sub-pixel cadence) == committed oracle frame."""
    import json
    pt = golden_tracer("tiny0", 32, 18, stack=16)
    p = api.InstanceConfig().pt_params(4242)
    p.stack_size, p.max_bounce, p.subpixel, p.tmp_lifetime, p.ray_tmin, p.clamp = 16, 5, 2, 2, 1e-4, 4.0
    p.sun[:] = [12.0, 11.0, 10.0]
    pt.SetConfig(p)
    cam = scenes._SCENE_TABLE["tiny0"][3]
    ip, iv = api.camera_matrices(cam["fov"], cam["yaw"], cam["pitch"], 32, 18)
    pt.SetCamera(ip, iv, cam["position"])
    pt.SetInstrumentation(counters=True)
    pt.Trace(True, 4)
    ref = np.load(os.path.join(GOLDEN, "tiny0_frame_32x18_4spp.npy"))
    assert np.array_equal(bits(pt.ReadResult()), bits(ref[..., :3]))
    st, gold = pt.GetStats(), json.load(open(os.path.join(GOLDEN, "tiny0_frame_32x18_4spp.json")))
    assert (st["rays"], st["nodes_visited"], st["tris_tested"], st["hits"], st["shaded"], st["max_stack"]) == \
        (gold["rays"], gold["nodes"], gold["tris"], gold["hits"], gold["shaded"], gold["max_depth"])
    assert pt.GetSPP() == 4


@pytest.mark.parametrize("name,w,h,spp", [("tiny2", 96, 64, 3), ("tiny1", 160, 90, 4), ("tiny0", 160, 90, 20), ("sibenik", 160, 90, 4),
                                          ("sponza", 192, 108, 4), ("tiny0", 100, 75, 5)])
def test_full_pipeline_bit_exact_vs_oracle(name, w, h, spp, scene_cache, sobol_matrices):
    inst = make_instance(scene_cache, name, w, h)
    c, pt = inst.m_config.c, inst.m_path_tracer
    osc, P = oracle_scene_from_instance(inst), oracle_params_from_config(c)
    for vt in (0, 1, 2, 4, 5):  # primaryray.glsl viewer types
        pt.m_viewer_type = vt
        pt.Trace(False)
        rgba, hits, _ = O.primary_frame(osc, P, vt)
        assert np.array_equal(bits(pt.ReadResult()), bits(rgba[..., :3])), "viewer type %d" % vt
    tri, uv = pt.ReadHits()
    assert np.array_equal(tri, hits["tri_id"])
    rays = random_rays(inst.scene.triangles, 20000, 3)
    gh, oh = pt.TraceRays(rays, with_stats=True), O.trace(osc, rays, c.stack_size)
    assert gh.tobytes() == oh.tobytes()  # ids, u/v/t bits, nodes visited, triangles tested, visit hash, max depth
    gh2 = pt.TraceRays(rays, with_stats=False)
    assert np.array_equal(gh2["tri_id"], oh["tri_id"]) and np.array_equal(bits(gh2["t"]), bits(oh["t"]))
    assert np.array_equal(bits(gh2["u"]), bits(oh["u"])) and np.array_equal(bits(gh2["v"]), bits(oh["v"]))
    pt.SetInstrumentation(counters=True)
    pt.ResetStats()
    pt.Trace(True, spp)
    st = O.PathTracerState(c.width, c.height)
    ost = O.pt_frames(osc, P, O.shift_bytes(99, c.width, c.height), sobol_matrices, st, spp).as_dict()
    assert np.array_equal(bits(pt.ReadResult()), bits(st.accum[..., :3]))
    g = pt.GetStats()
    assert (g["rays"], g["nodes_visited"], g["tris_tested"], g["hits"], g["shaded"], g["max_stack"]) == \
        (ost["rays"], ost["nodes"], ost["tris"], ost["hits"], ost["shaded"], ost["max_depth"])
    # progressive: more frames continue the same sequence (Sobol stream, spp counter, running mean)
    pt.Trace(True, 2)
    O.pt_frames(osc, P, O.shift_bytes(99, c.width, c.height), sobol_matrices, st, 2)
    assert np.array_equal(bits(pt.ReadResult()), bits(st.accum[..., :3])) and pt.GetSPP() == spp + 2
    # Trace(false) then Trace(true) restarts the accumulation like the reference (OglPathTracer.cpp:39-46,55-56)
    pt.Trace(False)
    assert pt.GetSPP() == 0
    pt.Trace(True, 1)
    st1 = O.PathTracerState(c.width, c.height)
    O.pt_frames(osc, P, O.shift_bytes(99, c.width, c.height), sobol_matrices, st1, 1)
    assert np.array_equal(bits(pt.ReadResult()), bits(st1.accum[..., :3]))


def test_ragged_and_edge_batches(scene_cache):
    inst = make_instance(scene_cache, "tiny0", 64, 48)
    pt = inst.m_path_tracer
    osc = oracle_scene_from_instance(inst)
    assert len(pt.TraceRays(np.zeros((0, 8), np.float32))) == 0  # empty batch
    for n in (1, 63, 64, 65, 4097):
        rays = random_rays(inst.scene.triangles, n, n)
        assert pt.TraceRays(rays, True).tobytes() == O.trace(osc, rays, inst.m_config.c.stack_size).tobytes()
    # more rays than the queue capacity (64x48 image -> 4096 slots): chunked internally
    rays = random_rays(inst.scene.triangles, 3 * 4096 + 17, 5)
    assert pt.TraceRays(rays, True).tobytes() == O.trace(osc, rays, inst.m_config.c.stack_size).tobytes()
    # NaN / Inf rays terminate and miss
    bad = random_rays(inst.scene.triangles, 256, 9)
    bad[:64, 0] = np.nan
    bad[64:128, 4] = np.nan
    bad[128:192, 1] = np.inf
    bad[192:, 4:7] = 0.0
    g, o = pt.TraceRays(bad, True), O.trace(osc, bad, inst.m_config.c.stack_size)
    assert np.array_equal(g["tri_id"], o["tri_id"]) and np.array_equal(g["nodes"], o["nodes"]) and np.array_equal(g["tris"], o["tris"])
    assert (g["tri_id"][:64] == -1).all() and (g["tri_id"][128:192] == -1).all()  # NaN / Inf origins can never hit


def test_stack_overflow_and_bad_material_are_reported(scene_cache):
    inst = make_instance(scene_cache, "tiny0", 64, 48, pt={"stackSize": 1})
    with pytest.raises(N.AdyptError) as e:
        inst.m_path_tracer.Trace(False)
    assert e.value.code == N.E_STACK_OVERFLOW
    # per-ray report in instrumented batches: max_depth = 0xffffffff, same rays as the oracle flags
    rays = random_rays(inst.scene.triangles, 5000, 1)
    g, o = inst.m_path_tracer.TraceRays(rays, True), O.trace(oracle_scene_from_instance(inst), rays, 1)
    assert np.array_equal(g["max_depth"], o["max_depth"]) and (g["max_depth"] == 0xFFFFFFFF).any()
    # material id -1 (faces before any usemtl, Scene.cpp:52): path ends, counted, no out-of-bounds read
    _, idx, nodes, tris, mats, woop = golden_scene("tiny1")
    tris = tris.copy()
    tris["matid"][::3] = -1
    tris["matid"][1::7] = 1000
    sc = api.Scene.FromArrays(tris, mats)
    b = api.WideBVH()
    b.nodes, b.tri_indices = nodes.view("u1").reshape(-1), idx
    hs = api.HipScene()
    hs.Initialize(sc, b)
    pt = api.HipPathTracer()
    pt.Initialize(api.InstanceConfig().pt_params(3), hs, 64, 36)
    cam = scenes._SCENE_TABLE["tiny1"][3]
    ip, iv = api.camera_matrices(cam["fov"], cam["yaw"], cam["pitch"], 64, 36)
    pt.SetCamera(ip, iv, cam["position"])
    pt.Trace(True, 2)
    assert pt.GetStats()["bad_materials"] > 0 and np.isfinite(pt.ReadResult()).all()


def test_tile_shards_reassemble_bit_exact(scene_cache):
    """Multi-GPU path on one GPU: contexts with tile_rank r of 3 render their blocks; untiled union == 1-context frame."""
    w, h, spp = 200, 120, 3
    full = make_instance(scene_cache, "tiny0", w, h, seed=5)
    full.m_path_tracer.Trace(True, spp)
    ref = full.m_path_tracer.ReadResult()
    out = np.zeros_like(ref)
    rays = 0
    for r in range(3):
        part = make_instance(scene_cache, "tiny0", w, h, seed=5, rank=r, world=3)
        part.m_path_tracer.Trace(True, spp)
        assert part.m_path_tracer.local_pixel_count() == D.block_count(w, h, r, 3) * 1024
        mine = part.m_path_tracer.ReadResult()
        mask = D.owner_mask(w, h, r, 3).astype(bool)
        assert (mine[~mask] == 0).all()
        out[mask] = mine[mask]
        rays += part.m_path_tracer.GetStats()["rays"]
    assert np.array_equal(bits(out), bits(ref))
    assert rays == full.m_path_tracer.GetStats()["rays"]


@pytest.mark.parametrize("world", [1, 3, 8])
def test_device_side_assembly_of_gathered_shards(world, scene_cache):
    """What rank 0 does after the one gather (adypt_assemble_radiance): the compact buffers of all ranks, laid out as the
    gather delivers them, are un-tiled on the device into the W x H x 3 image == the 1-context frame."""
    import torch
    w, h, spp = 200, 120, 2
    full = make_instance(scene_cache, "tiny0", w, h, seed=5)
    full.m_path_tracer.Trace(True, spp)
    ref = full.m_path_tracer.ReadResult()
    n = D.max_block_count(w, h, world) * D.BLOCK_PIXELS * 4
    gathered = torch.full((world * n,), float("nan"), dtype=torch.float32, device="cuda")
    parts = [make_instance(scene_cache, "tiny0", w, h, seed=5, rank=r, world=world) for r in range(world)]
    for r, part in enumerate(parts):
        part.m_path_tracer.Trace(True, spp)
        part.m_path_tracer.copy_local_radiance(gathered[r * n:(r + 1) * n].data_ptr(), n // 4)
    rgb = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    parts[0].m_path_tracer.assemble_radiance(gathered.data_ptr(), n // 4, rgb.data_ptr())
    assert np.array_equal(bits(rgb.cpu().numpy()), bits(ref))
    if world == 1:  # the single-process path of bench.py
        img = D.gather_radiance_device(gathered, parts[0].m_path_tracer, w, h, 0, 1)
        assert np.array_equal(bits(img.cpu().numpy()), bits(ref))


def test_async_enqueue_of_several_contexts_from_one_thread(scene_cache):
    """adypt_trace_spp_async / adypt_wait: one host thread keeps several contexts (here the two tile shards of one image,
    on the same GPU) busy at once; results equal the synchronous calls, errors surface at adypt_wait."""
    w, h, spp = 256, 144, 9
    full = make_instance(scene_cache, "tiny0", w, h, seed=5, pt={"tmpLifetime": 4})
    full.m_path_tracer.Trace(True, spp)
    ref = full.m_path_tracer.ReadResult()
    parts = [make_instance(scene_cache, "tiny0", w, h, seed=5, rank=r, world=2, pt={"tmpLifetime": 4}) for r in range(2)]
    for p in parts:
        p.m_path_tracer.SetFramesInFlight(2)  # several batches per call: enqueueing must not wait for the previous batch
        p.m_path_tracer.TraceAsync(spp - 4)
    for p in parts:
        p.m_path_tracer.TraceAsync(4)
    out = np.zeros_like(ref)
    for r, p in enumerate(parts):
        p.m_path_tracer.Wait()
        assert p.m_path_tracer.GetSPP() == spp
        mask = D.owner_mask(w, h, r, 2).astype(bool)
        out[mask] = p.m_path_tracer.ReadResult()[mask]
    assert np.array_equal(bits(out), bits(ref))
    # a stack overflow raised by asynchronous work is reported by Wait()
    bad = make_instance(scene_cache, "sibenik", 64, 36, pt={"stackSize": 1})
    bad.m_path_tracer.TraceAsync(1)
    with pytest.raises(N.AdyptError) as e:
        bad.m_path_tracer.Wait()
    assert e.value.code == N.E_STACK_OVERFLOW


def test_instance_update_loop_without_a_window(scene_cache, sobol_matrices):
    """Instance::Update (src/Instance.cpp:44-57) driven by explicit input state: viewer frames follow the moving camera
    (Camera::Control -> SetCamera -> Trace(false)), then path tracing starts from where the camera stopped."""
    inst = make_instance(scene_cache, "tiny0", 96, 64, seed=8, pt={"maxBounce": 4})
    K = api.Camera
    start = np.array(list(inst.m_config.c.position), dtype=np.float32)
    for _ in range(3):
        inst.Update(False, keys=K.KEY_W | K.KEY_A | K.KEY_SPACE, mouse=(6.0, -4.0), frame_seconds=0.125)
    c = inst.m_config.c
    assert not np.array_equal(np.array(list(c.position), dtype=np.float32), start)
    osc, P = oracle_scene_from_instance(inst), oracle_params_from_config(c)   # the config now holds the moved camera
    rgba, _, _ = O.primary_frame(osc, P, 0)
    assert np.array_equal(bits(inst.m_path_tracer.ReadResult()), bits(rgba[..., :3]))
    inst.Update(True, 4)
    st = O.PathTracerState(c.width, c.height)
    O.pt_frames(osc, P, O.shift_bytes(8, c.width, c.height), sobol_matrices, st, 4)
    assert np.array_equal(bits(inst.m_path_tracer.ReadResult()), bits(st.accum[..., :3]))
    assert inst.m_path_tracer.GetSPP() == 4


def test_full_size_frame_bit_exact_and_deterministic(scene_cache, sobol_matrices):
    """BASELINE config 2/3 size (1920x1080, sponza stand-in, 8 bounces): primary hits and one path-traced frame equal
    the oracle pixel for pixel; re-running gives identical bits; rays are counted exactly."""
    inst = make_instance(scene_cache, "sponza", 1920, 1080, seed=12345)
    c, pt = inst.m_config.c, inst.m_path_tracer
    osc, P = oracle_scene_from_instance(inst), oracle_params_from_config(c)
    pt.m_viewer_type = 0
    pt.Trace(False)
    rgba, hits, ost = O.primary_frame(osc, P, 0)
    tri, _ = pt.ReadHits()
    assert np.array_equal(tri, hits["tri_id"])
    assert np.array_equal(bits(pt.ReadResult()), bits(rgba[..., :3]))
    pt.ResetStats()
    pt.Trace(True, 1)
    a = pt.ReadResult()
    st = O.PathTracerState(c.width, c.height)
    os_ = O.pt_frames(osc, P, O.shift_bytes(12345, c.width, c.height), sobol_matrices, st, 1).as_dict()
    assert np.array_equal(bits(a), bits(st.accum[..., :3]))
    assert pt.GetStats()["rays"] == os_["rays"]
    pt.Reset()
    pt.Trace(True, 1)
    assert np.array_equal(bits(pt.ReadResult()), bits(a))
    # size-independent properties: clamp respected, finite, A never written to RGB, misses carry exactly the sun colour
    assert np.isfinite(a).all() and a.max() <= c.clamp
    sky = hits["tri_id"] == -1
    if sky.any():
        assert np.array_equal(a[sky], np.broadcast_to(np.minimum(np.array(list(c.sun), np.float32), np.float32(c.clamp)), a[sky].shape))


def test_bench_path_batched_1080p_spanning_two_tmplifetime_groups(scene_cache, sobol_matrices):
    """Exactly what bench.py times (its scene, its .config parameters, the default 32 frames in flight): a warm-up call of
    5 frames, then ONE call of 20 frames = frames 5..24 of the sequence.  That batch spans two tmpLifetime groups (frame 16
    re-traces its primaries): primary-only pass (k_trace_camera) into the second cache slice -> every frame starts from the
    cache of its group -> k_resolve in frame order -> image 1 = the last group's hits (tracer.hip adypt_trace_spp_async).
    Against the oracle's frame-by-frame loop (pathtracer.glsl:113-127, OglPathTracer.cpp:34-61), every pixel, every bit."""
    pt_cfg = {"maxBounce": 8, "subpixel": 8, "tmpLifetime": 16, "clamp": 4.0, "sun": [12.0, 11.0, 10.0], "stackSize": 24}  # = bench.py
    inst = make_instance(scene_cache, "sponza", 1920, 1080, pt=pt_cfg, seed=12345)
    c, pt = inst.m_config.c, inst.m_path_tracer
    assert pt.GetFramesInFlight() == 32 and c.tmp_lifetime == 16
    osc, P = oracle_scene_from_instance(inst), oracle_params_from_config(c)
    pt.ResetStats()
    pt.Trace(True, 5)
    pt.Trace(True, 20)
    a = pt.ReadResult()
    tri, uv = pt.ReadHits()
    st = O.PathTracerState(c.width, c.height)
    ost = O.pt_frames(osc, P, O.shift_bytes(12345, c.width, c.height), sobol_matrices, st, 25).as_dict()
    assert np.array_equal(bits(a), bits(st.accum[..., :3]))
    assert pt.GetStats()["rays"] == ost["rays"] and pt.GetSPP() == 25
    assert np.array_equal(tri, st.cache_tri)  # the primary hits of frame 16 (sub-pixel offset of group 1)
    m = tri >= 0
    assert np.array_equal(bits(uv)[m], bits(st.cache_uv)[m])


def test_exr_output_of_a_render(scene_cache, tmp_path):
    inst = make_instance(scene_cache, "tiny0", 96, 64)
    inst.m_path_tracer.Trace(True, 2)
    p = str(tmp_path / "r.exr")
    inst.m_path_tracer.SaveResult(p, False)
    assert np.array_equal(bits(api.load_exr(p)), bits(inst.m_path_tracer.ReadResult()))


def test_cli_headless_instance(scene_cache, tmp_path):
    import subprocess
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=48)
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    out = str(tmp_path / "cli.exr")
    r = subprocess.run([exe, spec.config_path, "--spp", "3", "--out", out, "--seed", "77"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=77)
    inst.m_path_tracer.Trace(True, 3)
    assert np.array_equal(bits(api.load_exr(out)), bits(inst.m_path_tracer.ReadResult()))


def test_cli_progressive_and_multi_device(scene_cache, tmp_path):
    """--save-every: the file on disk after every K samples is a complete image, the last one equals a straight render;
    --devices: the library's multi-device boundary behind the same command line (here three shards on the one GPU of the box)."""
    import subprocess
    spec = scenes.make_scene("tiny0", scene_cache, width=100, height=75)
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=5)
    inst.m_path_tracer.Trace(True, 7)
    want, shown = inst.m_path_tracer.ReadResult(), inst.m_path_tracer.ReadDisplay()
    for tag, extra, env in (("one", ["--device", "0"], {}), ("three", ["--devices", "0,0,0", "--test-hooks"], {"ADYPT_MULTI_SHARED_DEVICE": "1"})):
        out, png = str(tmp_path / (tag + ".exr")), str(tmp_path / (tag + ".png"))
        r = subprocess.run([exe, spec.config_path, "--spp", "7", "--save-every", "3", "--out", out, "--preview", png, "--seed", "5"] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, **env))
        log = r.stdout.decode()
        assert r.returncode == 0, log
        assert "3 spp saved" in log and "6 spp saved" in log and ("on 3 GPUs" if tag == "three" else "on 1 GPU,") in log, log
        assert np.array_equal(bits(api.load_exr(out)), bits(want))
        assert np.array_equal(api.load_image_rgb8(png), shown[..., :3])
        assert not os.path.exists(out + ".part") and not os.path.exists(png + ".part")
    # (a list that is none: tests/test_cli_options.py)
    r = subprocess.run([exe, spec.config_path, "--devices", "0,0", "--spp", "1", "--out", str(tmp_path / "dup.exr")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env={k: v for k, v in os.environ.items() if k != "ADYPT_MULTI_SHARED_DEVICE"})
    assert r.returncode == 1 and b"device listed twice" in r.stdout


@pytest.mark.parametrize("viewer", [0, 1, 2, 4, 5])
def test_display_transform_matches_oracle(viewer, scene_cache, sobol_matrices):
    """adypt_read_display = shaders/screen.glsl over the result image (f4): every byte equals the oracle's."""
    inst = make_instance(scene_cache, "tiny0", 100, 75, pt={"maxBounce": 4})
    pt = inst.m_path_tracer
    c = inst.m_config.c
    osc, P = oracle_scene_from_instance(inst), oracle_params_from_config(c)
    pt.m_viewer_type = viewer
    pt.Trace(False)
    rgba, _, _ = O.primary_frame(osc, P, viewer)
    assert np.array_equal(pt.ReadDisplay(), O.display(rgba, viewer))
    if viewer == 0:
        pt.Trace(True, 3)  # path-traced radiance is shown with uType = 3 (gamma)
        st = O.PathTracerState(c.width, c.height)
        O.pt_frames(osc, P, O.shift_bytes(99, c.width, c.height), sobol_matrices, st, 3)
        acc = st.accum.copy()
        acc[..., 3] = 1.0
        shown = pt.ReadDisplay()
        assert np.array_equal(shown, O.display(acc, 3))
        assert shown[..., :3].max() > 100  # not a black frame
