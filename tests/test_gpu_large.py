"""BASELINE.json's large configurations on the GPU (SURVEY.md §8c "maximum sizes"): the ~1.2 M-triangle stand-in at
4096x4096 (config 5: 'salle-de-bain' is not redistributable, `scenes.make_scene("salle")` is the same generator as
the bench scene at higher tessellation) against the oracle, plus the size-independent properties: determinism, tile
shards reassembling, frames-in-flight invariance, ray conservation."""
import numpy as np
import pytest

from adypt_amd import distributed as D
from oracle import oracle_py as O
from tests.helpers import (TMIN_CLASSES, bits, check_against_fp64_truth, mixed_rays, oracle_params_from_config,
                           oracle_scene_from_instance, random_rays, tmin_class)
from tests.test_gpu_parity import make_instance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def salle(scene_cache):
    return make_instance(scene_cache, "salle", 4096, 4096, seed=777)


def test_salle_random_rays_bit_exact(salle):
    osc = oracle_scene_from_instance(salle)
    rays = random_rays(salle.scene.triangles, 400000, 3)
    g = salle.m_path_tracer.TraceRays(rays, with_stats=True)
    o = O.trace(osc, rays, salle.m_config.c.stack_size)
    assert g.tobytes() == o.tobytes()
    assert (g["tri_id"] >= 0).mean() > 0.5  # the rays really exercise the hierarchy
    ga = salle.m_path_tracer.TraceRays(rays, with_stats=True, any_hit=True)
    assert ga.tobytes() == O.trace(osc, rays, salle.m_config.c.stack_size, any_hit=True).tobytes()


def test_salle_4096_frame_bit_exact(salle, sobol_matrices):
    c, pt = salle.m_config.c, salle.m_path_tracer
    osc, P = oracle_scene_from_instance(salle), oracle_params_from_config(c)
    pt.Reset()
    pt.ResetStats()
    pt.Trace(True, 2)
    a = pt.ReadResult()
    st = O.PathTracerState(c.width, c.height)
    ost = O.pt_frames(osc, P, O.shift_bytes(777, c.width, c.height), sobol_matrices, st, 2).as_dict()
    assert np.array_equal(bits(a), bits(st.accum[..., :3]))
    gst = pt.GetStats()
    assert gst["rays"] == ost["rays"] and gst["stack_overflows"] == 0
    assert np.isfinite(a).all() and a.max() <= c.clamp
    # determinism and frames-in-flight invariance at this size
    auto = pt.GetFramesInFlight()
    pt.SetFramesInFlight(1 if auto != 1 else 2)
    pt.Reset()
    pt.Trace(True, 2)
    assert np.array_equal(bits(pt.ReadResult()), bits(a))
    pt.SetFramesInFlight(auto)


def test_salle_4096_shards_reassemble(salle, scene_cache):
    pt = salle.m_path_tracer
    pt.Reset()
    pt.ResetStats()
    pt.Trace(True, 1)
    ref, rays_full = pt.ReadResult(), pt.GetStats()["rays"]
    w = h = 4096
    out, rays = np.zeros_like(ref), 0
    for r in range(2):
        part = make_instance(scene_cache, "salle", w, h, seed=777, rank=r, world=2)
        part.m_path_tracer.Trace(True, 1)
        mask = D.owner_mask(w, h, r, 2).astype(bool)
        out[mask] = part.m_path_tracer.ReadResult()[mask]
        rays += part.m_path_tracer.GetStats()["rays"]
        part.m_path_tracer.destroy()
    assert np.array_equal(bits(out), bits(ref)) and rays == rays_full


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE.json config 4: "San Miguel (~10M tri) 1920x1080 16spp, pixel-tile shard ... + radiance gather".  The asset is
# not available anywhere; scenes.make_scene("sanmiguel") is the ~10 M-triangle stand-in.  Its BVH
# (0.6 GB of nodes + Woop triangles) does not fit the 256 MB Infinity Cache: the only configuration whose traversal is
# HBM resident.
# ---------------------------------------------------------------------------------------------------------------------
def shard_tracer(inst, rank, world, seed):
    """A second context on the same host arrays (no second OBJ load / BVH build) rendering rank's blocks of a world-way shard."""
    from adypt_amd import api
    c = inst.m_config
    pt = api.HipPathTracer()
    pt.Initialize(c.pt_params(seed), inst.m_hipscene, c.m_width, c.m_height, 0, rank, world)
    ip, iv = inst.m_camera.matrices()
    pt.SetCamera(ip, iv, inst.m_camera.position)
    return pt


@pytest.fixture(scope="module")
def sanmiguel(scene_cache):
    inst = make_instance(scene_cache, "sanmiguel", 1920, 1080, seed=4242)
    assert inst.scene.n_tris > 9_000_000
    return inst


def test_sanmiguel_10M_random_rays_closest_and_any_bit_exact(sanmiguel):
    osc = oracle_scene_from_instance(sanmiguel)
    rays = random_rays(sanmiguel.scene.triangles, 250000, 5)
    pt, stack = sanmiguel.m_path_tracer, sanmiguel.m_config.c.stack_size
    g = pt.TraceRays(rays, with_stats=True)
    assert g.tobytes() == O.trace(osc, rays, stack).tobytes()  # ids, u/v/t bits, nodes, triangles, visit hash, max depth
    assert (g["tri_id"] >= 0).mean() > 0.5 and g["nodes"].mean() > 6
    ga = pt.TraceRays(rays, with_stats=True, any_hit=True)
    assert ga.tobytes() == O.trace(osc, rays, stack, any_hit=True).tobytes()
    # the non-instrumented kernel (the one the bench times) returns the same hits
    g2 = pt.TraceRays(rays, with_stats=False)
    assert np.array_equal(g2["tri_id"], g["tri_id"]) and np.array_equal(bits(g2["t"]), bits(g["t"]))
    assert np.array_equal(bits(g2["u"]), bits(g["u"])) and np.array_equal(bits(g2["v"]), bits(g["v"]))


def test_sanmiguel_10M_mixed_tmin_rays_bit_exact_and_against_fp64(sanmiguel):
    """tmin per ray varying inside every wave (tests/test_gpu_ray_tmin.py) on 10 M triangles; a subsample against the binary64 truth."""
    osc = oracle_scene_from_instance(sanmiguel)
    pt, stack = sanmiguel.m_path_tracer, sanmiguel.m_config.c.stack_size
    rays = mixed_rays(sanmiguel.scene.triangles, 100000, 9, lambda r: O.trace(osc, r, stack))
    g = pt.TraceRays(rays, with_stats=True)
    assert g.tobytes() == O.trace(osc, rays, stack).tobytes()
    ga = pt.TraceRays(rays, with_stats=True, any_hit=True)
    assert ga.tobytes() == O.trace(osc, rays, stack, any_hit=True).tobytes()
    g2 = pt.TraceRays(rays, with_stats=False)
    for k in ("tri_id", "u", "v", "t"):
        assert g2[k].tobytes() == g[k].tobytes(), k
    sub = slice(0, 1000)  # 1000 rays x 10 M triangles in binary64
    excused = check_against_fp64_truth(sanmiguel.scene.triangles, rays[sub], g2[sub])
    boundary = np.isin(tmin_class(len(rays))[sub], [TMIN_CLASSES.index(k) for k in ("at_hit", "above_hit", "below_hit")])
    assert excused[~boundary].mean() < 2e-3


def test_sanmiguel_10M_1080p_8_bounce_frames_bit_exact(sanmiguel, sobol_matrices):
    c, pt = sanmiguel.m_config.c, sanmiguel.m_path_tracer
    assert (c.width, c.height, c.max_bounce) == (1920, 1080, 8)
    osc, P = oracle_scene_from_instance(sanmiguel), oracle_params_from_config(c)
    pt.Reset()
    pt.SetInstrumentation(counters=True)
    pt.ResetStats()
    pt.Trace(True, 2)  # frame 0 traces its primaries, frame 1 starts from the cached hits; one batch
    a = pt.ReadResult()
    st = O.PathTracerState(c.width, c.height)
    ost = O.pt_frames(osc, P, O.shift_bytes(4242, c.width, c.height), sobol_matrices, st, 2).as_dict()
    assert np.array_equal(bits(a), bits(st.accum[..., :3]))
    g = pt.GetStats()
    assert (g["rays"], g["nodes_visited"], g["tris_tested"], g["hits"], g["shaded"]) == (ost["rays"], ost["nodes"], ost["tris"], ost["hits"], ost["shaded"])
    assert g["stack_overflows"] == 0 and np.isfinite(a).all() and a.max() <= c.clamp and a.mean() > 0.01
    pt.SetInstrumentation(False, False)


def test_sanmiguel_10M_two_way_tile_shards_reassemble(sanmiguel):
    pt = sanmiguel.m_path_tracer
    pt.Reset()
    pt.ResetStats()
    pt.Trace(True, 2)
    ref, rays_full = pt.ReadResult(), pt.GetStats()["rays"]
    w, h = 1920, 1080
    out, rays = np.zeros_like(ref), 0
    for r in range(2):
        part = shard_tracer(sanmiguel, r, 2, 4242)
        part.Trace(True, 2)
        mask = D.owner_mask(w, h, r, 2).astype(bool)
        img = part.ReadResult()
        assert not img[~mask].any()  # a shard only writes the blocks it owns
        out[mask] = img[mask]
        rays += part.GetStats()["rays"]
        part.destroy()
    assert np.array_equal(bits(out), bits(ref)) and rays == rays_full
