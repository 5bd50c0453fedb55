"""-m gpu: a PLOC tree built on the device with large triangles split into several references first (include/adypt_hip.h adypt_rebuild_bvh_ploc_split;
csrc/device/build.hip, the definition csrc/device/presplit.hpp).  The device's node, index, Woop and reference-box arrays are held against the host's
adypt_bvh_build_ploc_split + adypt_woop_matrices byte for byte (and that against numpy, binary64 and the SBVH tree in tests/test_presplit_definition.py);
rays and images after a rebuild against the CPU oracle on the host-built split tree, bit for bit.  The shapes are the smallest at which the kernels can
go wrong: beams(8, 4) is 136 triangles, three workgroups of the splitting kernels with a ragged last one and one block of the scan; beams(24, 8) is
1 168, nineteen workgroups and a scan across blocks; the soup is 5 000 triangles of similar size, where the level search has little to choose from."""
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
from tests.test_gpu_rebuild_ploc import host_ploc, levels_of  # noqa: E402
from tests.test_gpu_refit import PT, SPP, case_of, oracle_image, pose, same_woop, tracer, update  # noqa: E402
from tests.test_ploc_definition import DEGENERATE  # noqa: E402
from tests.test_presplit_definition import beams, lib_refs  # noqa: E402
from tests.test_refit_definition import lib_refit, same_bytes  # noqa: E402

_shapes, _split, _images = {}, {}, {}


class Shape(Loose):
    """a Loose case with the SBVH tree a context is created on"""

    def __init__(self, tris):
        super().__init__(tris)
        self._bvh = None

    def bvh(self, depth):
        if self._bvh is None:
            self._bvh = api.WideBVH()
            self._bvh.Build(self.scene, api.InstanceConfig().bvh_params())
        return self._bvh


def shape_of(name, cache):
    if name == "soup":
        return case_of("soup", cache)
    if name not in _shapes:
        tris = np.array(beams(*(int(x) for x in name[5:].split("x"))))
        tris.setflags(write=False)
        _shapes[name] = Shape(tris)
    return _shapes[name]


def host_split(case, name, which, budget):
    """(WideBVH.BuildPLOC(split_budget=budget) of the pose, its triangles, their Woop data, the level); shared and never written"""
    if (name, which, budget) not in _split:
        tris = case.tris if which == "rest" else pose(case.tris)
        b = api.WideBVH()
        b.BuildPLOC(api.Scene.FromArrays(tris, case.scene.materials), api.InstanceConfig().bvh_params(), 8, budget)
        b.nodes.setflags(write=False)
        _split[name, which, budget] = (b, tris, api.woop_matrices(tris, b.tri_indices), lib_refs(tris, budget)[0])
    return _split[name, which, budget]


def holds_split(p, b, woop):
    boxes = p.ReadRefBoxes()
    return holds(p, b, woop) and boxes is not None and boxes.shape == b.ref_boxes.shape and np.array_equal(bits(boxes), bits(b.ref_boxes))


CASES = [(name, budget) for name in ("beams8x4", "beams24x8", "soup") for budget in (0.1, 0.3)] + [("beams8x4", 1.0)]


@pytest.mark.parametrize("name,budget", CASES)
def test_device_equals_host(name, budget, scene_cache):
    case = shape_of(name, scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    for which in ("rest", "wave"):
        if which == "wave":
            update(p, pose(case.tris))
        info = p.RebuildBVH(method="ploc", split_budget=budget)
        b, tris, woop, level = host_split(case, name, which, budget)
        n_refs = len(b.tri_indices)
        print("%s %s budget %.1f: level %d, %d references of %d triangles" % (name, which, budget, level, n_refs, len(tris)))
        assert n_refs > len(tris), "the case splits something"
        assert p.GetBVHSizes() == (len(b.nodes) // 80, n_refs) == (info["n_nodes"], info["n_refs"])
        assert holds_split(p, b, woop), which
        assert info["levels"] == levels_of(b) and info["binary_depth"] >= info["levels"] - 1
        got_level, n_split = p.GetRebuildPresplit()
        assert got_level == level and n_split == (np.bincount(b.tri_indices, minlength=len(tris)) > 1).sum()
        ms = p.GetRebuildTiming()
        assert len(ms) == 7 and ms["total"] > 0.0 and all(ms[k] >= 0.0 for k in ms) and ms["bottom_up"] == 0.0 and ms["keys"] > 0.0
    p.destroy()


@pytest.mark.parametrize("name", ["beams24x8", "soup"])
def test_budget_zero_is_the_ploc_rebuild(name, scene_cache):
    case = shape_of(name, scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    b, tris, woop = host_ploc(case, name, "rest")
    info = p.RebuildBVH(method="ploc", split_budget=0.0)
    assert holds(p, b, woop) and p.ReadRefBoxes() is None and info["n_refs"] == len(tris) and p.GetRebuildPresplit() == (-1, 0)
    # the entry point itself, with a budget of 0
    r = N.RebuildInfo()
    c = p._contexts()[0]
    N.check(N.lib.adypt_rebuild_bvh_ploc_split(c, None, 8, 0.0, N.C.byref(r)), c)
    assert holds(p, b, woop) and p.ReadRefBoxes() is None and (r.n_nodes, r.n_refs) == (info["n_nodes"], info["n_refs"]) and p.GetRebuildPresplit() == (-1, 0)
    p.destroy()


def test_split_unsplit_and_linear_share_the_scratch(scene_cache):
    case = shape_of("beams24x8", scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    lin, _, lin_woop = host_linear(case, "beams24x8", "rest")
    un, _, un_woop = host_ploc(case, "beams24x8", "rest")
    b, _, woop, _ = host_split(case, "beams24x8", "rest", 0.3)
    small, _, small_woop, _ = host_split(case, "beams24x8", "rest", 0.1)
    p.RebuildBVH(method="ploc", split_budget=0.3)
    assert holds_split(p, b, woop)
    p.RebuildBVH(method="ploc")
    assert holds(p, un, un_woop) and p.ReadRefBoxes() is None and p.GetRebuildPresplit() == (-1, 0)
    p.RebuildBVH(method="ploc", split_budget=0.1)
    assert holds_split(p, small, small_woop)
    p.RebuildBVH()
    assert holds(p, lin, lin_woop) and p.ReadRefBoxes() is None
    p.RebuildBVH(method="ploc", split_budget=0.3)
    assert holds_split(p, b, woop)
    with pytest.raises(ValueError):
        p.RebuildBVH(method="linear", split_budget=0.3)
    assert holds_split(p, b, woop)
    p.destroy()


@pytest.mark.parametrize("what", sorted(DEGENERATE))
def test_degenerate_inputs(what):
    tris = DEGENERATE[what]()
    case = Loose(tris)
    sbvh = api.WideBVH()
    cfg = api.InstanceConfig().bvh_params()
    sbvh.Build(case.scene, cfg)
    b = api.WideBVH()
    b.BuildPLOC(case.scene, cfg, 8, 1.0)
    p = tracer(case, case.scene, sbvh)
    info = p.RebuildBVH(method="ploc", split_budget=1.0)
    assert holds(p, b, api.woop_matrices(tris, b.tri_indices))
    boxes = p.ReadRefBoxes()
    assert (boxes is None and len(b.ref_boxes) == 0) or np.array_equal(bits(boxes), bits(b.ref_boxes))
    assert (info["n_nodes"], info["n_refs"], info["levels"]) == (len(b.nodes) // 80, len(b.tri_indices), levels_of(b))
    assert p.GetRebuildPresplit()[0] == lib_refs(tris, 1.0)[0]
    rays = np.zeros((len(tris) + 7, 8), np.float32)
    rays[:, :3], rays[:, 3] = (37.0, 41.0, 43.0), 1e-4
    rays[:len(tris), 4:7] = (tris["p"][:, 0].astype(np.float64) * 0.25 + tris["p"].astype(np.float64).mean(axis=1) * 0.75) - np.array([37.0, 41.0, 43.0])
    rays[len(tris):, 4:7] = (1.0, 0.5, 0.25)  # away from everything
    got, want = p.TraceRays(rays, with_stats=True), O.trace(O.Scene(b.nodes, b.tri_indices, tris, case.scene.materials), rays, stack_size=PT["stack_size"])
    for f in api.HIT_DT.names:
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    assert (want["tri_id"][:len(tris)] >= 0).sum() >= max(1, len(tris) // 2) and (want["tri_id"][len(tris):] < 0).all()
    p.destroy()


@pytest.mark.parametrize("name", ["beams8x4", "beams24x8", "soup"])
def test_rays_after_a_rebuild(name, scene_cache):
    case = shape_of(name, scene_cache)
    b, tris, woop, _ = host_split(case, name, "wave", 0.3)
    osc = O.Scene(b.nodes, b.tri_indices, tris, case.scene.materials, woop=woop)
    rays = T.rays_in_box(tris, 4096)
    p = tracer(case, case.scene, case.bvh(48))
    update(p, tris)
    p.RebuildBVH(method="ploc", split_budget=0.3)
    for any_hit in (False, True):
        got, want = p.TraceRays(rays, with_stats=True, any_hit=any_hit), O.trace(osc, rays, stack_size=PT["stack_size"], any_hit=any_hit)
        for f in api.HIT_DT.names:
            assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), "%s (any_hit %s)" % (f, any_hit)
        assert (want["tri_id"] >= 0).sum() > 1000
    p.destroy()


def split_image(case, name, sobol_matrices):
    if name not in _images:
        b, tris, _, _ = host_split(case, name, "wave", 0.3)
        _images[name] = oracle_image(case, b.nodes, b.tri_indices, tris, sobol_matrices)
        _images[name].setflags(write=False)
    return _images[name]


@pytest.mark.parametrize("variant", ["fused", "launch_per_bounce", "fused_remap"])
def test_image_after_a_rebuild(variant, scene_cache, sobol_matrices, monkeypatch):
    case = shape_of("beams8x4", scene_cache)
    if variant.endswith("remap"):
        monkeypatch.setenv("ADYPT_REF_TRIANGLES_MAX_MB", "0")  # no per-reference records: k_path remaps through the new index array
    p = tracer(case, case.scene, case.bvh(48))
    fused = variant.startswith("fused")
    if not fused:
        p.SetFusedBounces(False)
    p.Trace(True, 2)  # (the old tree has been rendered: per-reference records, primary-hit cache and image are its)
    update(p, pose(case.tris))
    p.RebuildBVH(method="ploc", split_budget=0.3)
    assert p.GetSPP() == 0
    p.Trace(True, SPP)
    assert p.GetFusedBounces() == fused
    want = split_image(case, "beams8x4", sobol_matrices)
    assert np.array_equal(bits(p.ReadResult()), bits(want)), "the image on the rebuilt tree"
    assert (want != 0).any()
    p.destroy()


@pytest.mark.parametrize("name", ["beams24x8", "soup"])
def test_update_after_a_split_rebuild(name, scene_cache):
    case = shape_of(name, scene_cache)
    b, _, _, _ = host_split(case, name, "rest", 0.3)
    p = tracer(case, case.scene, case.bvh(48))
    p.RebuildBVH(method="ploc", split_budget=0.3)
    assert p.ReadRefBoxes() is not None
    moved = T.jitter(case.tris)
    update(p, moved)
    r, want = lib_refit(b.nodes, b.tri_indices, moved)
    assert r == N.ADYPT_OK
    nodes, woop = p.ReadBVH()
    assert same_bytes(nodes, want) and same_woop(woop, api.woop_matrices(moved, b.tri_indices)) and np.array_equal(p.ReadTriIndices(), b.tri_indices)
    assert p.ReadRefBoxes() is None  # whole triangles from here on
    p.destroy()


def test_two_shards_on_one_device(scene_cache, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = shape_of("soup", scene_cache)
    b, tris, woop, level = host_split(case, "soup", "wave", 0.3)
    n_refs = len(b.tri_indices)
    w, h = 64, 36  # 2 x 2 blocks: both shards own some
    single = tracer(case, case.scene, case.bvh(48), w, h)
    multi = tracer(case, case.scene, case.bvh(48), w, h, cls=api.MultiPathTracer, devices=(0, 0))
    assert multi.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in multi._contexts())
    for t in (single, multi):
        t.Trace(True, 2)
        update(t, tris)
        info = t.RebuildBVH(method="ploc", split_budget=0.3)
        assert t.GetSPP() == 0 and info["n_refs"] == n_refs and t.GetRebuildPresplit()[0] == level
        t.Trace(True, SPP)
    assert holds_split(single, b, woop)
    a = single.ReadBVH()
    for c in multi._contexts():  # every device rebuilt its own copy
        nodes, got_woop, idx, boxes = np.zeros_like(a[0]), np.zeros_like(a[1]), np.zeros(n_refs, np.int32), np.zeros((n_refs, 6), np.float32)
        N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, got_woop.ctypes.data), c)
        N.check(N.lib.adypt_read_tri_indices(c, idx.ctypes.data), c)
        assert N.lib.adypt_read_ref_boxes(c, boxes.ctypes.data) == n_refs
        assert same_bytes(nodes, a[0]) and np.array_equal(bits(got_woop), bits(a[1])) and np.array_equal(idx, b.tri_indices) and np.array_equal(bits(boxes), bits(b.ref_boxes))
    assert np.array_equal(bits(multi.ReadResult()), bits(single.ReadResult()))
    assert not np.array_equal(bits(single.ReadResult()), np.zeros_like(bits(single.ReadResult())))
    multi.destroy()
    single.destroy()


def test_refusals_change_nothing(scene_cache):
    case = shape_of("beams8x4", scene_cache)
    p = tracer(case, case.scene, case.bvh(48))
    p.Trace(True, SPP)
    image, before, idx = p.ReadResult(), p.ReadBVH(), p.ReadTriIndices()

    def untouched():
        now = p.ReadBVH()
        return (same_bytes(now[0], before[0]) and np.array_equal(bits(now[1]), bits(before[1])) and np.array_equal(p.ReadTriIndices(), idx)
                and p.GetSPP() == SPP and np.array_equal(bits(p.ReadResult()), bits(image)) and p.ReadRefBoxes() is None)

    for budget in (-0.1, 1.5, float("nan")):
        with pytest.raises(N.AdyptError) as e:
            p.RebuildBVH(None, "ploc", 8, budget)
        assert e.value.code == N.E_INVALID and untouched()
    with pytest.raises(N.AdyptError) as e:
        p.RebuildBVH(None, "ploc", 40, 0.3)
    assert e.value.code == N.E_INVALID and untouched()
    with pytest.raises(ValueError):
        p.RebuildBVH(None, "linear", 8, 0.3)
    with pytest.raises(N.AdyptError) as e:
        p.GetRebuildPresplit()  # nothing has been rebuilt
    assert e.value.code == N.E_STATE and untouched()
    # and the scene rebuilds
    p.RebuildBVH(method="ploc", split_budget=0.3)
    b, _, woop, _ = host_split(case, "beams8x4", "rest", 0.3)
    assert holds_split(p, b, woop)
    p.destroy()


def test_cli_split_budget(scene_cache, tmp_path):
    """adypt_hip --rebuild-method ploc --split-budget B renders on the tree RebuildBVH(method="ploc", split_budget=B) builds in this process, and says so"""
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=5)
    pt = inst.m_path_tracer
    info = pt.RebuildBVH(inst.m_config.bvh_params(), "ploc", 8, 0.3)
    level = pt.GetRebuildPresplit()[0]
    assert info["n_refs"] > 554
    pt.Trace(True, 3)
    want = pt.ReadResult()
    pt.destroy()
    out = str(tmp_path / "split.exr")
    r = subprocess.run([exe, spec.config_path, "--rebuild-method", "ploc", "--split-budget", "0.3", "--spp", "3", "--seed", "5", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = r.stdout.decode()
    assert r.returncode == 0, log
    assert "rebuild: %d nodes, %d references, %d levels, method ploc radius 8 split budget 0.3 level %d" % (info["n_nodes"], info["n_refs"], info["levels"], level) in log, log
    assert np.array_equal(bits(api.load_exr(out)), bits(want))
    # (a budget without --rebuild-method ploc: tests/test_cli_options.py)
    r = subprocess.run([exe, spec.config_path, "--rebuild-method", "ploc", "--split-budget", "1.5", "--spp", "1", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 1 and "budget" in r.stdout.decode()
