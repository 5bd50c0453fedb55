"""-m gpu: tmin, per ray and per pass.  Every other test traces at tmin 1e-4 only, so a kernel that used the wrong lane's tmin, its own
tmin for another lane's triangle (traverse_trip.inc, section B: the tester pulls the owner's tmin through the crossbar) or a literal in
place of the pass's value would pass them all.  Here:
  - ray batches (k_trace, closest and any hit, instrumented and not) whose tmin changes from lane to lane (tests/helpers.py: mixed_rays),
    bit-exact with the oracle, the same records for a shuffled batch, and on sponza against the binary64 truth directly;
  - the pass's rayTMin at 0, at a value beyond some pixels' first surface, and at 1e-4, through the camera kernel (every viewer
    type), the one-launch and the launch-per-bounce pipelines, sun-visibility queries, several frames in flight and look-ahead —
    bit-exact with the oracle, and visibly different from the 1e-4 render;
  - a new rayTMin handed over mid-run: it takes effect at the next first frame only (OglPathTracer.cpp:39-46)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests.helpers import (TMIN_CLASSES, bits, check_against_fp64_truth, mixed_rays, oracle_params_from_config,  # noqa: E402
                           oracle_scene_from_instance, tmin_class)

SEED = 31
COUNTS = (("rays", "rays"), ("nodes_visited", "nodes"), ("tris_tested", "tris"), ("shaded", "shaded"))
BOUNDARY = [TMIN_CLASSES.index(k) for k in ("at_hit", "above_hit", "below_hit")]


def _instance(cache, name, w, h, pt):
    spec = scenes.make_scene(name, cache, width=w, height=h, pt=pt)
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=SEED), api.InstanceConfig.last_error()
    return inst


def _params(c, tmin=None, sun=False):
    ip, iv = O.camera(c.fov, c.yaw, c.pitch, c.width, c.height)
    return O.make_params(c.width, c.height, list(c.position), ip, iv, stack_size=c.stack_size, max_bounce=c.max_bounce,
                         subpixel=c.subpixel, tmp_life=c.tmp_lifetime, tmin=c.ray_tmin if tmin is None else tmin, clamp=c.clamp,
                         sun=list(c.sun), sun_visibility=sun)


def _check_batch(pt, osc, rays, stack):
    """Both kernels of a ray batch against the oracle; returns the records (closest, any)."""
    out = []
    for any_hit in (False, True):
        oh = O.trace(osc, rays, stack, any_hit=any_hit)
        gh = pt.TraceRays(rays, with_stats=True, any_hit=any_hit)
        assert gh.tobytes() == oh.tobytes(), "instrumented kernel, any_hit=%s: %d rays differ" % (any_hit, (gh != oh).sum())
        g2 = pt.TraceRays(rays, with_stats=False, any_hit=any_hit)
        assert np.array_equal(g2["tri_id"], oh["tri_id"]), "kernel of the bench, any_hit=%s: triangles" % any_hit
        for k in ("u", "v", "t"):
            assert np.array_equal(bits(g2[k]), bits(oh[k])), "kernel of the bench, any_hit=%s: %s" % (any_hit, k)
        assert np.array_equal(g2["ref_idx"], np.where(oh["tri_id"] == -1, -1, 0))  # adypt_trace_rays without stats: -1 / 0
        out.append(g2)
    return out


@pytest.mark.parametrize("name,n", [("tiny0", 20000), ("sibenik", 30000), ("sponza", 30000)])
def test_ray_batches_with_mixed_tmin_bit_exact(name, n, scene_cache):
    inst = _instance(scene_cache, name, 64, 36, None)
    pt, stack = inst.m_path_tracer, inst.m_config.c.stack_size
    osc = oracle_scene_from_instance(inst)
    rays = mixed_rays(inst.scene.triangles, n, 11, lambda r: O.trace(osc, r, stack))
    closest, anyh = _check_batch(pt, osc, rays, stack)
    tc = tmin_class(n)
    assert (closest["tri_id"][tc == TMIN_CLASSES.index("negative")] >= 0).mean() > 0.2
    assert (closest["tri_id"][tc == TMIN_CLASSES.index("beyond")] == -1).all()
    if name == "sponza":
        # the kernel itself against the binary64 truth, not through the restatement
        sub = slice(0, 4000)
        for hits, any_hit in ((closest, False), (anyh, True)):
            excused = check_against_fp64_truth(inst.scene.triangles, rays[sub], hits[sub], any_hit=any_hit)
            assert excused[~np.isin(tc[sub], BOUNDARY)].mean() < 1e-3


def test_shuffled_batch_returns_the_same_records(scene_cache):
    """A ray's record does not depend on which rays share its wave: catches a lane reading another lane's state without the oracle."""
    inst = _instance(scene_cache, "sibenik", 64, 36, None)
    pt, stack = inst.m_path_tracer, inst.m_config.c.stack_size
    osc = oracle_scene_from_instance(inst)
    rays = mixed_rays(inst.scene.triangles, 30000, 12, lambda r: O.trace(osc, r, stack))
    perm = np.random.RandomState(5).permutation(len(rays))
    for any_hit in (False, True):
        for stats in (True, False):
            a = pt.TraceRays(rays, with_stats=stats, any_hit=any_hit)
            b = pt.TraceRays(rays[perm], with_stats=stats, any_hit=any_hit)
            assert a[perm].tobytes() == b.tobytes(), "any_hit=%s stats=%s" % (any_hit, stats)


def _primary_t_percentile(cache, name, w, h, pt_cfg, q=5):
    """a tmin beyond the first surface of about q % of the pixels (the oracle's primary hits at tmin 1e-4)"""
    spec = scenes.make_scene(name, cache, width=w, height=h, pt=dict(pt_cfg, rayTMin=1e-4))
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=SEED), api.InstanceConfig.last_error()
    _, hits, _ = O.primary_frame(oracle_scene_from_instance(inst), _params(inst.m_config.c), 0)
    return float(np.float32(np.percentile(hits["t"][hits["tri_id"] >= 0], q)))


def _render_everywhere(cache, name, w, h, pt_cfg, sobol_matrices, spp=4):
    """One instance at pt_cfg's rayTMin through every kernel that takes the pass's tmin; each bit-exact with the oracle."""
    inst = _instance(cache, name, w, h, pt_cfg)
    c, p = inst.m_config.c, inst.m_path_tracer
    osc = oracle_scene_from_instance(inst)
    assert np.float32(c.ray_tmin) == np.float32(pt_cfg["rayTMin"])
    P = _params(c)
    # primary-only frames: k_trace_camera with the viewer's colour, then the hit cache (ReadHits)
    for vt in (0, 1, 2, 4, 5):
        p.m_viewer_type = vt
        p.Trace(False)
        rgba, ph, _ = O.primary_frame(osc, P, vt)
        assert np.array_equal(bits(p.ReadResult()), bits(rgba[..., :3])), "viewer type %d" % vt
    tri, uv = p.ReadHits()
    assert np.array_equal(tri, ph["tri_id"])
    m = tri >= 0
    assert np.array_equal(bits(uv[..., 0])[m], bits(ph["u"])[m]) and np.array_equal(bits(uv[..., 1])[m], bits(ph["v"])[m])
    shift = O.shift_bytes(SEED, c.width, c.height)
    want = {}
    for sun in (False, True):
        st = O.PathTracerState(c.width, c.height)
        ost = O.pt_frames(osc, _params(c, sun=sun), shift, sobol_matrices, st, spp).as_dict()
        want[sun] = (st, ost)
    # (fused, sun visibility, frames in flight, look-ahead)
    runs = [(True, False, 1, False), (False, False, 1, False), (True, True, 1, False), (False, True, 1, False),
            (True, False, 3, False), (False, True, 3, False), (True, False, 3, True), (True, True, 2, True)]
    out = None
    for fused, sun, fif, look in runs:
        what = "fused=%s sun=%s frames_in_flight=%d lookahead=%s" % (fused, sun, fif, look)
        p.SetLookahead(False)
        p.SetFramesInFlight(fif)
        p.SetLookahead(look)
        p.SetFusedBounces(fused)
        p.SetSunVisibility(sun)
        p.SetInstrumentation(counters=not look)
        p.Reset()
        p.ResetStats()
        if look:
            for _ in range(spp):
                p.Trace(True, 1)
        else:
            p.Trace(True, spp)
        st, ost = want[sun]
        img = p.ReadResult()
        assert np.array_equal(bits(img), bits(st.accum[..., :3])), what + ": image"
        tri, uv = p.ReadHits()
        assert np.array_equal(tri, st.cache_tri), what + ": primary-hit cache"
        m = tri >= 0
        assert np.array_equal(bits(uv)[m], bits(st.cache_uv)[m]), what + ": primary-hit cache (u, v)"
        if not look:
            g = p.GetStats()
            for gk, ok in COUNTS:
                assert g[gk] == ost[ok], (what, gk, g[gk], ost[ok])
        if out is None:
            out = {"primary_tri": ph["tri_id"], "img": img, "stats": {k: ost[k] for _, k in COUNTS}}
    return out


@pytest.mark.parametrize("name,w,h", [("tiny0", 96, 64), ("sibenik", 128, 72)])
def test_pass_tmin_reaches_every_kernel(name, w, h, scene_cache, sobol_matrices):
    pt_cfg = {"tmpLifetime": 2, "maxBounce": 5, "subpixel": 2}
    large = _primary_t_percentile(scene_cache, name, w, h, pt_cfg)
    assert large > 1e-3
    r = {t: _render_everywhere(scene_cache, name, w, h, dict(pt_cfg, rayTMin=t), sobol_matrices) for t in (1e-4, 0.0, large)}
    ref = r[1e-4]
    # the large value moves primary hits (through the wall); 0 moves the bounces (a bounce's ray may find its own surface again)
    assert (r[large]["primary_tri"] != ref["primary_tri"]).mean() > 0.01
    assert r[0.0]["stats"] != ref["stats"] or not np.array_equal(bits(r[0.0]["img"]), bits(ref["img"]))


def test_new_tmin_is_handed_over_at_the_next_first_frame(scene_cache, sobol_matrices):
    """SetConfig while frames are being accumulated (look-ahead on: frames are already traced ahead): the frames that follow keep the
    old rayTMin until Reset, then the new one holds (OglPathTracer.cpp:39-46: update_config_args at the first frame only)."""
    pt_cfg = {"tmpLifetime": 2, "maxBounce": 5, "subpixel": 2, "rayTMin": 1e-4}
    new = _primary_t_percentile(scene_cache, "tiny0", 96, 64, pt_cfg, q=10)
    inst = _instance(scene_cache, "tiny0", 96, 64, pt_cfg)
    c, p = inst.m_config.c, inst.m_path_tracer
    osc = oracle_scene_from_instance(inst)
    shift = O.shift_bytes(SEED, c.width, c.height)
    p.SetFramesInFlight(3)
    p.SetLookahead(True)

    def frames(P, state, k, what):
        for i in range(k):
            p.Trace(True, 1)
            O.pt_frames(osc, P, shift, sobol_matrices, state, 1)
            assert np.array_equal(bits(p.ReadResult()), bits(state.accum[..., :3])), "%s, frame %d" % (what, i)
            tri, uv = p.ReadHits()
            assert np.array_equal(tri, state.cache_tri), "%s, frame %d: primary-hit cache" % (what, i)

    old_state = O.PathTracerState(c.width, c.height)
    frames(_params(c), old_state, 2, "before SetConfig")
    cfg = inst.m_config.pt_params(SEED)
    cfg.ray_tmin = new
    p.SetConfig(cfg)
    frames(_params(c), old_state, 4, "after SetConfig, before Reset")
    p.Reset()
    new_state = O.PathTracerState(c.width, c.height)
    frames(_params(c, tmin=new), new_state, 4, "after Reset")
    assert (new_state.cache_tri != old_state.cache_tri).mean() > 0.01  # the new value did change the primary hits
