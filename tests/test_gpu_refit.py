"""-m gpu: moving geometry on the device (include/adypt_hip.h adypt_update_triangles ...; csrc/device/refit.hip).  The device's node and Woop arrays are
held against the host's adypt_bvh_refit + adypt_woop_matrices byte for byte (and those against numpy in tests/test_refit_definition.py); rays and
images after an update against the CPU oracle on the host-refitted arrays, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import refit_truth as T  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_refit_definition import lib_refit, same_bytes  # noqa: E402

SEED = 5
W, H, SPP = 32, 18, 4
PT = dict(stack_size=32, max_bounce=4, subpixel=3, tmp_life=16)
_cases = {}


class Case:
    """A rest pose with its camera: api.Scene (textures included), TRI_DT triangles, the trees built from it"""

    def __init__(self, name, cache):
        if name == "soup":
            # 5 000 triangles: levels whose node counts are no multiples of 32 and span several workgroups, a reference count that is no multiple of 256
            self.scene = api.Scene.FromArrays(T.soup(5000), T.soup_material())
            self.ip, self.iv = api.camera_matrices(60.0, 30.0, -10.0, W, H)
            self.pos = np.zeros(3, np.float32)
        else:
            spec = scenes.make_scene(name, cache, width=W, height=H)
            cfg = api.InstanceConfig()
            assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
            self.scene = api.Scene()
            assert self.scene.LoadFromFile(cfg.m_obj_filename)
            self.ip, self.iv = api.camera_matrices(cfg.c.fov, cfg.c.yaw, cfg.c.pitch, W, H)
            self.pos = np.array(list(cfg.c.position), np.float32)
        self.tris = np.array(self.scene.triangles).view(O.TRI_DT)
        self.tris.setflags(write=False)
        self._bvh = {}

    def bvh(self, depth):
        if depth not in self._bvh:
            cfg = api.InstanceConfig().bvh_params()
            cfg.max_spatial_depth = depth
            b = api.WideBVH()
            b.Build(self.scene, cfg)
            b.nodes.setflags(write=False)
            self._bvh[depth] = b
        return self._bvh[depth]

    def moved_scene(self, tris):
        """api.Scene of the same materials and textures with other triangles"""
        s = api.Scene()
        s.triangles, s.materials, s.textures = np.ascontiguousarray(tris).view(np.uint8).reshape(-1), self.scene.materials, self.scene.textures
        return s


def case_of(name, cache):
    if name not in _cases:
        _cases[name] = Case(name, cache)
    return _cases[name]


def params():
    p = api.InstanceConfig().pt_params(SEED)
    p.stack_size, p.max_bounce, p.subpixel, p.tmp_lifetime = PT["stack_size"], PT["max_bounce"], PT["subpixel"], PT["tmp_life"]
    return p


def tracer(case, scene, bvh, w=W, h=H, cls=api.HipPathTracer, **kw):
    hs = api.HipScene()
    hs.Initialize(scene, bvh)
    p = cls()
    p.Initialize(params(), hs, w, h, **kw)
    ip, iv = (case.ip, case.iv) if (w, h) == (W, H) else api.camera_matrices(60.0, 30.0, -10.0, w, h)
    p.SetCamera(ip, iv, case.pos)
    return p


def pose(tris, normals=False):
    t = T.wave(tris)
    if normals:  # other normals too: tilted and normalised again
        n = t["n"].astype(np.float64) + np.array([0.3, -0.2, 0.1])
        t["n"] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    return t


def update(p, moved, normals=False, first=0, count=None):
    count = len(moved) - first if count is None else count
    sl = slice(first, first + count)
    p.UpdateTriangles(first, moved["p"][sl].reshape(-1, 9), moved["n"][sl].reshape(-1, 9) if normals else None)


def same_woop(got, want):
    """The device's Woop array is the host's bit for bit — except in the 12 floats of a degenerate triangle, which are NaN on both sides and may differ
    in the NaN's sign and payload: IEEE 754 leaves those of a generated NaN open, x86 makes 0xffc00000 (and flips it under negation), gfx950 0x7fc00000.
    Such a reference can never be hit on either side.  Which entries are NaN must agree exactly."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def host_refit(case, depth, moved):
    b = case.bvh(depth)
    r, nodes = lib_refit(b.nodes, b.tri_indices, moved)
    assert r == N.ADYPT_OK
    return nodes, api.woop_matrices(moved, b.tri_indices)


def oracle_image(case, nodes, tri_indices, tris, sobol_matrices, sun_visibility=False, ip=None, iv=None, w=W, h=H):
    osc = O.Scene(nodes, tri_indices, tris, case.scene.materials, textures=case.scene.textures)
    c = api.InstanceConfig().c
    P = O.make_params(w, h, list(case.pos), case.ip if ip is None else ip, case.iv if iv is None else iv, stack_size=PT["stack_size"], max_bounce=PT["max_bounce"],
                      subpixel=PT["subpixel"], tmp_life=PT["tmp_life"], tmin=c.ray_tmin, clamp=c.clamp, sun=list(c.sun), sun_visibility=sun_visibility)
    st = O.PathTracerState(w, h)
    O.pt_frames(osc, P, O.shift_bytes(SEED, w, h), sobol_matrices, st, SPP)
    return st.accum[..., :3].copy()


@pytest.mark.parametrize("name", ["tiny2", "tiny0", "soup"])
def test_device_equals_host(name, scene_cache):
    case = case_of(name, scene_cache)
    # spatial splits, the wave pose
    b = case.bvh(48)
    moved = pose(case.tris)
    p = tracer(case, case.scene, b)
    update(p, moved)
    nodes, woop = p.ReadBVH()
    want_nodes, want_woop = host_refit(case, 48, moved)
    assert same_bytes(nodes, want_nodes), "nodes after the wave pose"
    assert same_woop(woop, want_woop), "Woop data after the wave pose"
    assert not same_bytes(nodes, b.nodes)
    ms = p.GetRefitTiming()
    assert ms["total"] > 0.0 and ms["nodes"] > 0.0
    # back in the rest pose the refit of the split tree is the host's again
    update(p, case.tris)
    nodes, woop = p.ReadBVH()
    want_nodes, want_woop = host_refit(case, 48, case.tris)
    assert same_bytes(nodes, want_nodes) and same_woop(woop, want_woop)
    p.destroy()
    # no spatial splits, unmoved: what was uploaded
    b = case.bvh(-1)
    p = tracer(case, case.scene, b)
    update(p, case.tris)
    nodes, woop = p.ReadBVH()
    assert same_bytes(nodes, b.nodes), "unmoved, unsplit: the builder's nodes"
    assert same_woop(woop, api.woop_matrices(case.tris, b.tri_indices))
    p.destroy()


@pytest.mark.parametrize("name", ["tiny2", "tiny0", "soup"])
def test_rays_after_an_update(name, scene_cache):
    case = case_of(name, scene_cache)
    b = case.bvh(48)
    moved = pose(case.tris)
    nodes, woop = host_refit(case, 48, moved)
    osc = O.Scene(nodes, b.tri_indices, moved, case.scene.materials, woop=woop)
    rays = T.rays_in_box(moved, 4096)
    p = tracer(case, case.scene, b)
    update(p, moved)
    for any_hit in (False, True):
        got, want = p.TraceRays(rays, with_stats=True, any_hit=any_hit), O.trace(osc, rays, stack_size=PT["stack_size"], any_hit=any_hit)
        for f in api.HIT_DT.names:
            assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), "%s (any_hit %s)" % (f, any_hit)
        assert name == "tiny2" or (want["tri_id"] >= 0).sum() > 1000  # (tiny2: five triangles, random rays miss them; the node counts still compare)
    p.destroy()


@pytest.mark.parametrize("variant", ["fused", "launch_per_bounce", "remap", "normals"])
@pytest.mark.parametrize("name", ["tiny0", "soup"])
def test_image_after_an_update(name, variant, scene_cache, sobol_matrices, monkeypatch):
    case = case_of(name, scene_cache)
    b = case.bvh(48)
    with_normals = variant == "normals"
    moved = pose(case.tris, with_normals)
    if variant == "remap":
        monkeypatch.setenv("ADYPT_REF_TRIANGLES_MAX_MB", "0")  # no per-reference records: k_path remaps through the index array
    p = tracer(case, case.scene, b)
    if variant == "launch_per_bounce":
        p.SetFusedBounces(False)
    p.Trace(True, 2)  # (the old pose has been rendered: per-reference records, primary-hit cache and image are its)
    update(p, moved, with_normals)
    assert p.GetSPP() == 0
    p.Trace(True, SPP)
    assert p.GetFusedBounces() == (variant != "launch_per_bounce")
    nodes, _ = host_refit(case, 48, moved)
    want = oracle_image(case, nodes, b.tri_indices, moved, sobol_matrices)
    assert np.array_equal(bits(p.ReadResult()), bits(want)), "the image of the moved scene"
    rest_image = oracle_image(case, b.nodes, b.tri_indices, case.tris, sobol_matrices)
    assert not np.array_equal(bits(want), bits(rest_image))  # the pose shows
    if with_normals:
        assert not np.array_equal(bits(want), bits(oracle_image(case, nodes, b.tri_indices, pose(case.tris), sobol_matrices)))  # ... and so do the normals
    p.destroy()


def fresh_image(case, moved, sun=False):
    """the image a context created for the moved pose (host-refitted tree) renders"""
    b = api.WideBVH()
    b.nodes, b.tri_indices = host_refit(case, 48, moved)[0], case.bvh(48).tri_indices
    p = tracer(case, case.moved_scene(moved), b)
    if sun:
        p.SetSunVisibility(True, [0.6, 1.0, 0.2])
    p.Trace(True, SPP)
    image = p.ReadResult()
    p.destroy()
    return image


@pytest.mark.parametrize("setting", ["frozen_blocks", "lookahead", "sun_query"])
def test_update_in_the_middle_of_an_accumulation(setting, scene_cache):
    case = case_of("tiny0", scene_cache)
    moved = pose(case.tris)
    p = tracer(case, case.scene, case.bvh(48))
    if setting == "frozen_blocks":
        p.SetNoiseStats(True)
        r = p.TraceAdaptive(1e30, min_spp=2, max_spp=8, check_every=2)  # every block is below the target at the first check
        assert r["blocks_frozen"] == r["blocks"] > 0 and (p.ReadBlockSPP()[1] == 2).all()
    elif setting == "lookahead":
        p.SetFramesInFlight(4)
        p.SetLookahead(True)
        p.Trace(True, 1)
        assert p.GetLookaheadFrames() == 3
    else:
        p.SetSunVisibility(True, [0.6, 1.0, 0.2])
        p.Trace(True, 3)
    update(p, moved)
    assert p.GetSPP() == 0 and p.GetLookaheadFrames() == 0
    if setting == "lookahead":
        for _ in range(SPP):
            p.Trace(True, 1)
    else:
        p.Trace(True, SPP)
    assert p.GetSPP() == SPP
    if setting == "frozen_blocks":
        assert (p.ReadBlockSPP()[1] == SPP).all()  # thawed
    assert np.array_equal(bits(p.ReadResult()), bits(fresh_image(case, moved, sun=setting == "sun_query"))), setting
    p.destroy()


def test_partial_ranges_and_a_bad_range(scene_cache):
    case = case_of("tiny0", scene_cache)
    moved = pose(case.tris, True)
    n = len(moved)
    whole, parts = tracer(case, case.scene, case.bvh(48)), tracer(case, case.scene, case.bvh(48))
    update(whole, moved, True)
    half = n // 2 + 1
    update(parts, moved, True, 0, half)
    update(parts, moved, True, half, n - half)
    a, b = whole.ReadBVH(), parts.ReadBVH()
    assert same_bytes(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))  # (device against device: NaNs included)
    for t in (whole, parts):
        t.Trace(True, SPP)
    image = whole.ReadResult()
    assert np.array_equal(bits(image), bits(parts.ReadResult()))
    parts.destroy()
    # refused: nothing changes, not even the accumulation
    pos = moved["p"].reshape(-1, 9)
    for first, count in ((1, n), (-1, 2), (n + 1, 0)):
        with pytest.raises(N.AdyptError) as e:
            whole.UpdateTriangles(first, pos[:count])
        assert e.value.code == N.E_INVALID
    assert N.lib.adypt_update_triangles(whole._ctx, 0, n, None, None) == N.E_INVALID
    assert whole.GetSPP() == SPP and np.array_equal(bits(whole.ReadResult()), bits(image))
    now = whole.ReadBVH()
    assert same_bytes(now[0], a[0]) and np.array_equal(bits(now[1]), bits(a[1]))
    whole.Reset()
    whole.Trace(True, SPP)
    assert np.array_equal(bits(whole.ReadResult()), bits(image))
    whole.destroy()


def test_two_shards_on_one_device(scene_cache, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = case_of("soup", scene_cache)
    moved = pose(case.tris, True)
    w, h = 64, 36  # 2 x 2 blocks: both shards own some
    single = tracer(case, case.scene, case.bvh(48), w, h)
    multi = tracer(case, case.scene, case.bvh(48), w, h, cls=api.MultiPathTracer, devices=(0, 0))
    assert multi.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in multi._contexts())
    for t in (single, multi):
        t.Trace(True, 2)
        update(t, moved, True)
        assert t.GetSPP() == 0
        t.Trace(True, SPP)
    a = single.ReadBVH()
    for c in multi._contexts():  # every device refitted its own copy
        nodes, woop = np.zeros_like(a[0]), np.zeros_like(a[1])
        N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, woop.ctypes.data), c)
        assert same_bytes(nodes, a[0]) and np.array_equal(bits(woop), bits(a[1]))
    assert np.array_equal(bits(multi.ReadResult()), bits(single.ReadResult()))
    assert not np.array_equal(bits(single.ReadResult()), np.zeros_like(bits(single.ReadResult())))
    with pytest.raises(N.AdyptError) as e:
        multi.UpdateTriangles(1, moved["p"].reshape(-1, 9))
    assert e.value.code == N.E_INVALID
    multi.destroy()
    single.destroy()
