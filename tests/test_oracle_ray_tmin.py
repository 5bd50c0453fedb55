"""The oracle's traversal (oracle/oracle.cpp) with a tmin per ray that varies inside every wave — 0, 1e-4, random, beyond the scene,
negative, and exactly the ray's own hit distance and its neighbours — and with directions at the ray setup's substitution
(traversal.glsl:16-19), against the binary64 truth (O.brute_force_ex).  CPU only: the GPU side is tests/test_gpu_ray_tmin.py."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests.helpers import (N_TMIN_CLASSES, TMIN_CLASSES, check_against_fp64_truth, cpu_scene, golden_scene, mixed_rays,
                           oracle_scene_from_golden, tmin_class)

BOUNDARY = [TMIN_CLASSES.index(k) for k in ("at_hit", "above_hit", "below_hit")]


def _cls(name):
    return TMIN_CLASSES.index(name)


@pytest.mark.parametrize("name,n", [("tiny0", 8000), ("sibenik", 6000), ("sponza", 3000)])
@pytest.mark.parametrize("any_hit", [False, True])
def test_oracle_agrees_with_fp64_truth_on_mixed_rays(name, n, any_hit, scene_cache):
    sc, _, osc = cpu_scene(scene_cache, name)
    rays = mixed_rays(sc.triangles, n, 17, lambda r: O.trace(osc, r, 24))
    hits = O.trace(osc, rays, 24, any_hit=any_hit)
    excused = check_against_fp64_truth(sc.triangles, rays, hits, any_hit=any_hit)
    # outside the classes that put tmin on the hit itself, binary32 and binary64 decide alike but for a rare edge graze
    tc = tmin_class(n)
    assert excused[~np.isin(tc, BOUNDARY)].mean() < 1e-3
    # every class is exercised: hits at tmin 0 / 1e-4 / random / negative, none beyond the scene
    for k in ("zero", "1e-4", "uniform", "negative"):
        assert (hits["tri_id"][tc == _cls(k)] >= 0).mean() > 0.2, k
    assert (hits["tri_id"][tc == _cls("beyond")] == -1).all()


@pytest.mark.parametrize("name", ["tiny0", "sibenik"])
def test_oracle_tmin_is_strict_at_the_hit_distance(name, scene_cache):
    """tmin = the float t of the ray's own closest hit: that hit is gone (t > tmin is strict, traversal.glsl:235); one float below it:
    the same hit again; and no record ever has t <= tmin."""
    sc, _, osc = cpu_scene(scene_cache, name)
    n = 8000
    rays = mixed_rays(sc.triangles, n, 23, lambda r: O.trace(osc, r, 24))
    first_rays = rays.copy()
    first_rays[:, 3] = 1e-4
    first = O.trace(osc, first_rays, 24)
    tc = tmin_class(n)
    for any_hit in (False, True):
        h = O.trace(osc, rays, 24, any_hit=any_hit)
        hit = h["tri_id"] >= 0
        assert (h["t"][hit] > rays[hit, 3]).all(), "a hit at t <= tmin"
        assert (h["t"][hit] < np.float32(1e9)).all()
        was = first["tri_id"] >= 0
        at = (tc == _cls("at_hit")) & was
        assert at.sum() > 200
        assert not ((h["tri_id"] == first["tri_id"]) & (h["t"] == first["t"]))[at].any(), "the hit at t == tmin was accepted"
        if not any_hit:
            below = (tc == _cls("below_hit")) & was
            same = (h["tri_id"] == first["tri_id"]) & (h["t"].view(np.uint32) == first["t"].view(np.uint32))
            # (a box whose binary32 exit lies below the hit's t culls it, as in the shader: an axis-aligned triangle on its box's face)
            assert same[below].mean() > 0.9, same[below].mean()
            assert (h["t"][(tc == _cls("at_hit")) & hit] > first["t"][(tc == _cls("at_hit")) & hit]).all()


@pytest.mark.parametrize("name", ["tiny0", "tiny1"])
def test_traversal_agrees_with_fp64_truth_on_reference_built_arrays_mixed_tmin(name):
    """test_oracle_golden.test_traversal_agrees_with_fp64_brute_force's scenes (the reference's own BVH and Woop arrays), mixed rays."""
    _, _, _, tris, _, _ = golden_scene(name)
    sc = oracle_scene_from_golden(name)
    rays = mixed_rays(tris, 6000, 123, lambda r: O.trace(sc, r, 32))
    tc = tmin_class(len(rays))
    for any_hit in (False, True):
        hits = O.trace(sc, rays, 32, any_hit=any_hit)
        excused = check_against_fp64_truth(tris, rays, hits, any_hit=any_hit)
        assert excused[~np.isin(tc, BOUNDARY)].mean() < 1e-3
        assert (hits["tri_id"][tc == _cls("negative")] >= 0).any()


def test_mixed_rays_mix_every_class_in_every_wave(scene_cache):
    sc, _, osc = cpu_scene(scene_cache, "tiny0")
    rays = mixed_rays(sc.triangles, 640, 1, lambda r: O.trace(osc, r, 24))
    tc = tmin_class(len(rays))
    for w in range(0, 640, 64):
        assert set(tc[w:w + 64]) == set(range(N_TMIN_CLASSES))
        assert len(np.unique(rays[w:w + 64, 3])) > 16
    d = rays[:, 4:7]
    ooeps = np.float32(2.0 ** -64)
    assert (d.view(np.uint32) == np.float32(-0.0).view(np.uint32)).any()
    assert (np.abs(d) == ooeps).any()
    assert (np.abs(d) == np.nextafter(ooeps, np.float32(0))).any() and (np.abs(d) == np.nextafter(ooeps, np.float32(1))).any()
    assert ((np.abs(d) > 0) & (np.abs(d) < np.finfo(np.float32).tiny)).any()
    assert ((np.abs(d) < ooeps).all(1) & (np.sign(d) < 0).any(1) & (np.sign(d) > 0).any(1)).any()
