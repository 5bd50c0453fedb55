"""-m gpu: a new tree built on the device by PLOC (include/adypt_hip.h adypt_rebuild_bvh_ploc; csrc/device/build.hip, the definition csrc/device/ploc.hpp).
The device's node, index and Woop arrays are held against the host's adypt_bvh_build_ploc + adypt_woop_matrices byte for byte (and that against numpy
and the SBVH tree in tests/test_ploc_definition.py); rays and images after a rebuild against the CPU oracle on the host-built PLOC tree, bit for bit.
The shapes are the smallest at which the kernels can go wrong: 5 000 triangles are 20 workgroups of the search (halos across workgroup boundaries, a
scan across blocks), 554 are three with a ragged last one, 5 and less are one."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import refit_truth as T  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_gpu_rebuild import Loose, holds, host_linear  # noqa: E402
from tests.test_gpu_refit import PT, SPP, case_of, oracle_image, pose, same_woop, tracer, update  # noqa: E402
from tests.test_ploc_definition import DEGENERATE  # noqa: E402
from tests.test_refit_definition import lib_refit, same_bytes  # noqa: E402

_ploc, _images = {}, {}


def host_ploc(case, name, which, radius=8):
    """(WideBVH.BuildPLOC of the pose, its triangles, their Woop data); shared and never written"""
    if (name, which, radius) not in _ploc:
        tris = case.tris if which == "rest" else pose(case.tris)
        b = api.WideBVH()
        b.BuildPLOC(api.Scene.FromArrays(tris, case.scene.materials), api.InstanceConfig().bvh_params(), radius)
        b.nodes.setflags(write=False)
        _ploc[name, which, radius] = (b, tris, api.woop_matrices(tris, b.tri_indices))
    return _ploc[name, which, radius]


def levels_of(b):
    return int(T.depths(np.ascontiguousarray(b.nodes).view(O.NODE_DT)).max()) + 1


@pytest.mark.parametrize("name", ["tiny2", "tiny0", "soup"])
def test_device_equals_host(name, scene_cache):
    case = case_of(name, scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    info = p.RebuildBVH(method="ploc")
    b, tris, woop = host_ploc(case, name, "rest")
    assert p.GetBVHSizes() == (len(b.nodes) // 80, len(tris)) == (info["n_nodes"], info["n_refs"])
    assert holds(p, b, woop), "the rest pose"
    assert info["levels"] == levels_of(b) and info["binary_depth"] >= info["levels"] - 1
    ms = p.GetRebuildTiming()
    assert len(ms) == 7 and ms["total"] > 0.0 and all(ms[k] >= 0.0 for k in ms) and ms["bottom_up"] == 0.0
    update(p, pose(case.tris))
    info = p.RebuildBVH(method="ploc", radius=8)
    b, tris, woop = host_ploc(case, name, "wave")
    assert holds(p, b, woop), "after the wave pose"
    assert p.GetBVHSizes() == (len(b.nodes) // 80, len(tris)) == (info["n_nodes"], info["n_refs"]) and info["levels"] == levels_of(b)
    p.destroy()


@pytest.mark.parametrize("radius", [1, 32])
def test_other_radii(radius, scene_cache):
    case = case_of("soup", scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    info = p.RebuildBVH(None, "ploc", radius)
    b, tris, woop = host_ploc(case, "soup", "rest", radius)
    assert holds(p, b, woop)
    assert (info["n_nodes"], info["n_refs"], info["levels"]) == (len(b.nodes) // 80, len(tris), levels_of(b))
    assert not same_bytes(b.nodes, host_ploc(case, "soup", "rest")[0].nodes)  # (another tree than radius 8's)
    p.destroy()


@pytest.mark.parametrize("what", sorted(DEGENERATE))
def test_degenerate_inputs(what):
    tris = DEGENERATE[what]()
    case = Loose(tris)
    sbvh = api.WideBVH()
    cfg = api.InstanceConfig().bvh_params()
    sbvh.Build(case.scene, cfg)
    b = api.WideBVH()
    b.BuildPLOC(case.scene, cfg)
    p = tracer(case, case.scene, sbvh)
    info = p.RebuildBVH(method="ploc")
    assert holds(p, b, api.woop_matrices(tris, b.tri_indices))
    assert (info["n_nodes"], info["n_refs"], info["levels"]) == (len(b.nodes) // 80, len(tris), levels_of(b))
    assert what != "one" or (info["n_nodes"], info["levels"], info["binary_depth"]) == (1, 1, 0)
    assert what != "two" or info["binary_depth"] == 1
    rays = np.zeros((len(tris) + 7, 8), np.float32)
    rays[:, :3], rays[:, 3] = (37.0, 41.0, 43.0), 1e-4
    rays[:len(tris), 4:7] = (tris["p"][:, 0].astype(np.float64) * 0.25 + tris["p"].astype(np.float64).mean(axis=1) * 0.75) - np.array([37.0, 41.0, 43.0])
    rays[len(tris):, 4:7] = (1.0, 0.5, 0.25)  # away from everything
    got, want = p.TraceRays(rays, with_stats=True), O.trace(O.Scene(b.nodes, b.tri_indices, tris, case.scene.materials), rays, stack_size=PT["stack_size"])
    for f in api.HIT_DT.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    assert (want["tri_id"][:len(tris)] >= 0).sum() >= max(1, len(tris) // 2) and (want["tri_id"][len(tris):] < 0).all()
    p.destroy()


@pytest.mark.parametrize("name", ["tiny2", "tiny0", "soup"])
def test_rays_after_a_rebuild(name, scene_cache):
    case = case_of(name, scene_cache)
    b, tris, woop = host_ploc(case, name, "wave")
    osc = O.Scene(b.nodes, b.tri_indices, tris, case.scene.materials, woop=woop)
    rays = T.rays_in_box(tris, 4096)
    p = tracer(case, case.scene, case.bvh(48))
    update(p, tris)
    p.RebuildBVH(method="ploc")
    for any_hit in (False, True):
        got, want = p.TraceRays(rays, with_stats=True, any_hit=any_hit), O.trace(osc, rays, stack_size=PT["stack_size"], any_hit=any_hit)
        for f in api.HIT_DT.names:
            assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), "%s (any_hit %s)" % (f, any_hit)
        assert name == "tiny2" or (want["tri_id"] >= 0).sum() > 1000
    p.destroy()


def ploc_image(case, name, sobol_matrices):
    if name not in _images:
        b, tris, _ = host_ploc(case, name, "wave")
        _images[name] = oracle_image(case, b.nodes, b.tri_indices, tris, sobol_matrices)
        _images[name].setflags(write=False)
    return _images[name]


@pytest.mark.parametrize("variant", ["fused", "launch_per_bounce", "fused_remap"])
def test_image_after_a_rebuild(variant, scene_cache, sobol_matrices, monkeypatch):
    case = case_of("tiny0", scene_cache)
    if variant.endswith("remap"):
        monkeypatch.setenv("ADYPT_REF_TRIANGLES_MAX_MB", "0")  # no per-reference records: k_path remaps through the new index array
    p = tracer(case, case.scene, case.bvh(48))
    fused = variant.startswith("fused")
    if not fused:
        p.SetFusedBounces(False)
    p.Trace(True, 2)  # (the old tree has been rendered: per-reference records, primary-hit cache and image are its)
    update(p, pose(case.tris))
    p.RebuildBVH(method="ploc")
    assert p.GetSPP() == 0
    p.Trace(True, SPP)
    assert p.GetFusedBounces() == fused
    assert np.array_equal(bits(p.ReadResult()), bits(ploc_image(case, "tiny0", sobol_matrices))), "the image on the rebuilt tree"
    p.destroy()


@pytest.mark.parametrize("name", ["tiny0", "soup"])
def test_refit_after_a_rebuild(name, scene_cache):
    case = case_of(name, scene_cache)
    b, _, _ = host_ploc(case, name, "rest")
    p = tracer(case, case.scene, case.bvh(48))
    p.RebuildBVH(method="ploc")
    moved = T.jitter(case.tris)
    update(p, moved)
    r, want = lib_refit(b.nodes, b.tri_indices, moved)
    assert r == N.ADYPT_OK
    nodes, woop = p.ReadBVH()
    assert same_bytes(nodes, want) and same_woop(woop, api.woop_matrices(moved, b.tri_indices)) and np.array_equal(p.ReadTriIndices(), b.tri_indices)
    p.destroy()


def test_linear_and_ploc_share_the_scratch(scene_cache):
    case = case_of("soup", scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    lin, _, lin_woop = host_linear(case, "soup", "rest")
    b, _, woop = host_ploc(case, "soup", "rest")
    p.RebuildBVH(method="ploc")
    assert holds(p, b, woop)
    p.RebuildBVH()  # the default is the linear tree, as ever
    assert holds(p, lin, lin_woop) and p.GetRebuildTiming()["bottom_up"] >= 0.0
    p.RebuildBVH(method="ploc")
    assert holds(p, b, woop)
    p.RebuildBVH(method="linear")
    assert holds(p, lin, lin_woop)
    with pytest.raises(ValueError):
        p.RebuildBVH(method="sah")
    assert holds(p, lin, lin_woop)
    p.destroy()


def test_two_shards_on_one_device(scene_cache, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = case_of("soup", scene_cache)
    b, tris, woop = host_ploc(case, "soup", "wave")
    w, h = 64, 36  # 2 x 2 blocks: both shards own some
    single = tracer(case, case.scene, case.bvh(48), w, h)
    multi = tracer(case, case.scene, case.bvh(48), w, h, cls=api.MultiPathTracer, devices=(0, 0))
    assert multi.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in multi._contexts())
    for t in (single, multi):
        t.Trace(True, 2)
        update(t, tris)
        info = t.RebuildBVH(method="ploc")
        assert t.GetSPP() == 0 and info["n_refs"] == len(tris)
        t.Trace(True, SPP)
    assert holds(single, b, woop)
    a = single.ReadBVH()
    for c in multi._contexts():  # every device rebuilt its own copy
        nodes, got_woop, idx = np.zeros_like(a[0]), np.zeros_like(a[1]), np.zeros(len(tris), np.int32)
        N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, got_woop.ctypes.data), c)
        N.check(N.lib.adypt_read_tri_indices(c, idx.ctypes.data), c)
        assert same_bytes(nodes, a[0]) and np.array_equal(bits(got_woop), bits(a[1])) and np.array_equal(idx, b.tri_indices)
    assert np.array_equal(bits(multi.ReadResult()), bits(single.ReadResult()))
    assert not np.array_equal(bits(single.ReadResult()), np.zeros_like(bits(single.ReadResult())))
    multi.destroy()
    single.destroy()


def test_refusals_change_nothing(scene_cache):
    case = case_of("tiny0", scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    p.Trace(True, SPP)
    image, before, idx = p.ReadResult(), p.ReadBVH(), p.ReadTriIndices()

    def refused(cfg, radius):
        with pytest.raises(N.AdyptError) as e:
            p.RebuildBVH(cfg, "ploc", radius)
        assert e.value.code == N.E_INVALID

    def untouched(before, idx):
        now = p.ReadBVH()
        return same_bytes(now[0], before[0]) and np.array_equal(bits(now[1]), bits(before[1])) and np.array_equal(p.ReadTriIndices(), idx)

    for radius in (0, 33):
        refused(None, radius)
    for tri_sah, node_sah in ((0.0, 1.0), (0.3, -1.0), (float("nan"), 1.0), (0.3, float("inf"))):
        cfg = api.InstanceConfig().bvh_params()
        cfg.triangle_sah, cfg.node_sah = tri_sah, node_sah
        refused(cfg, 8)
    with pytest.raises(N.AdyptError) as e:
        p.GetRebuildTiming()  # nothing has been rebuilt
    assert e.value.code == N.E_STATE
    assert p.GetSPP() == SPP and np.array_equal(bits(p.ReadResult()), bits(image)) and untouched(before, idx)
    # a NaN vertex, written by UpdateTriangles: the update itself refits the old tree and starts the image again; the rebuild then refuses the scene
    broken = np.array(case.tris)
    broken["p"][7] = np.nan
    update(p, broken)
    p.Trace(True, 1)
    image_broken, before_broken = p.ReadResult(), p.ReadBVH()
    refused(None, 8)
    assert p.GetSPP() == 1 and np.array_equal(bits(p.ReadResult()), bits(image_broken)) and untouched(before_broken, idx)
    # the old tree is in place and usable: back in the rest pose it renders what a context that was only ever refitted renders
    update(p, case.tris)
    p.Trace(True, SPP)
    q = tracer(case, case.scene, case.bvh(48))
    update(q, case.tris)
    q.Trace(True, SPP)
    assert untouched(q.ReadBVH(), idx) and np.array_equal(bits(p.ReadResult()), bits(q.ReadResult()))
    q.destroy()
    # and the scene rebuilds once it is whole again
    p.RebuildBVH(method="ploc")
    b, _, woop = host_ploc(case, "tiny0", "rest")
    assert holds(p, b, woop)
    p.destroy()


def test_cli_rebuild_method(scene_cache, tmp_path):
    """adypt_hip --rebuild-method ploc --ploc-radius R renders on the tree RebuildBVH(method="ploc", radius=R) builds in this process, and says so"""
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=5)
    pt = inst.m_path_tracer
    info = pt.RebuildBVH(inst.m_config.bvh_params(), "ploc", 4)
    pt.Trace(True, 3)
    want = pt.ReadResult()
    pt.destroy()
    out = str(tmp_path / "ploc.exr")
    r = subprocess.run([exe, spec.config_path, "--rebuild-method", "ploc", "--ploc-radius", "4", "--spp", "3", "--seed", "5", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = r.stdout.decode()
    assert r.returncode == 0, log
    assert "rebuild: %d nodes, 554 references, %d levels, method ploc radius 4" % (info["n_nodes"], info["levels"]) in log, log
    assert np.array_equal(bits(api.load_exr(out)), bits(want))
    r = subprocess.run([exe, spec.config_path, "--rebuild-method", "ploc", "--ploc-radius", "40", "--spp", "1", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 1 and "radius" in r.stdout.decode()
    # (a method that is none: tests/test_cli_options.py)
