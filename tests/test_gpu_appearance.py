"""-m gpu: materials, textures and triangle attributes changed on the device (include/adypt_hip.h adypt_set_materials, adypt_update_texture,
adypt_set_triangle_attributes; csrc/device/appearance.hip).  The device's table, arena and records are held byte for byte against a context that
adypt_create made of the same arrays, against the numpy restatements (tests/appearance_truth.py, tests/tri_record_truth.py) and against the host's
adypt_pack_appearance; images after a change against the CPU oracle on the new arrays, bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import appearance_truth as A  # noqa: E402
from tests import tri_record_truth as R  # noqa: E402
from tests import test_gpu_refit as G  # noqa: E402
from tests.helpers import bits  # noqa: E402
from tests.test_appearance_definition import SIZES, materials as numbered_materials, texture, textures_of  # noqa: E402
from tests.test_tri_record_definition import class_soup  # noqa: E402

W, H, SPP, PT, SEED = G.W, G.H, G.SPP, G.PT, G.SEED
_images = {}


def flat(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def scene_of(tris, mats, textures):
    s = api.Scene()
    s.triangles, s.materials, s.textures = flat(tris), flat(mats), list(textures)
    return s


def index_of(mats, kd):
    hit = np.flatnonzero((np.abs(mats["kd"] - np.array(kd, np.float32)) < 1e-6).all(axis=1))
    assert len(hit) == 1, kd
    return int(hit[0])


def new_table(case, glow=True):
    """The new surfaces of a tiny scene: the lamp dark, `white` a glossy illum 2 / Ns 200 (class words flip), `red` with a 5 x 3 texture, and one more
    material than before; (materials, textures).  At 32 x 18 and 4 spp nothing but an emitter lights these scenes (an escaping path brings nothing
    back, and tiny1 has no lamp at all), so with the lamp dark the image is black and would show none of the other changes: `glow` switches `green` on
    as a lamp, which lights the floor and the walls in both scenes.  glow False is the table without it."""
    old = np.array(case.scene.materials).view(O.MAT_DT)
    m = np.zeros(len(old) + 1, dtype=O.MAT_DT)
    m[:-1] = old
    m["ke"][:-1][old["ke"].any(axis=1)] = 0.0
    white, red = index_of(old, (0.75, 0.75, 0.75)), index_of(old, (0.75, 0.15, 0.15))
    m["illum"][white], m["shininess"][white], m["ks"][white] = 2, 200.0, (0.5, 0.5, 0.5)
    m["dtex"][red] = 0
    if glow:
        m["ke"][index_of(old, (0.15, 0.75, 0.15))] = (6.0, 5.0, 4.0)
    m[-1] = old[red]
    m["kd"][-1] = (0.2, 0.3, 0.9)
    return m, [texture(5, 3, 40)]


def oracle_image(case, depth, tris, mats, textures, sobol_matrices, sun_visibility=False, key=None):
    if key is not None and key in _images:
        return _images[key]
    b = case.bvh(depth)
    osc = O.Scene(b.nodes, b.tri_indices, tris, mats, textures=textures)
    c = api.InstanceConfig().c
    P = O.make_params(W, H, list(case.pos), case.ip, case.iv, stack_size=PT["stack_size"], max_bounce=PT["max_bounce"], subpixel=PT["subpixel"], tmp_life=PT["tmp_life"],
                      tmin=c.ray_tmin, clamp=c.clamp, sun=list(c.sun), sun_visibility=sun_visibility)
    st = O.PathTracerState(W, H)
    O.pt_frames(osc, P, O.shift_bytes(SEED, W, H), sobol_matrices, st, SPP)
    image = st.accum[..., :3].copy()
    image.setflags(write=False)
    if key is not None:
        _images[key] = image
    return image


def state_of(p):
    return p.ReadMaterialRecords().tobytes(), p.ReadTexels().tobytes(), p.ReadTriangleRecords().tobytes()


# ---- 1. device state equals a fresh context ----
@pytest.mark.parametrize("shade_bin", [False, True])
def test_state_equals_a_fresh_context(shade_bin, scene_cache, monkeypatch):
    if shade_bin:
        monkeypatch.setenv("ADYPT_SHADE_BIN", "1")
    case = G.case_of("tiny0", scene_cache)
    mats, tex = new_table(case, glow=False)
    p = G.tracer(case, case.scene, case.bvh(48))
    before = p.ReadTriangleRecords()
    assert p.ReadMaterialRecords().tobytes() == A.records(case.scene.materials, case.scene.textures).tobytes()  # (what adypt_create made)
    p.Trace(True, 2)
    info = p.SetMaterials(mats, tex)
    assert info["n_mats"] == len(mats) and info["n_textures"] == 1 and info["n_texels"] == 6 * 3 and info["device_bytes"] > 0
    white = index_of(np.array(case.scene.materials).view(O.MAT_DT), (0.75, 0.75, 0.75))
    assert info["reclassed"] == (case.tris["matid"] == white).sum() > 0
    assert p.GetSPP() == 0
    fresh = G.tracer(case, scene_of(case.tris, mats, tex), case.bvh(48))
    got, want = state_of(p), state_of(fresh)
    fresh.destroy()
    want_rec, want_texels, _ = A.pack(mats, tex)
    host = api.pack_appearance(mats, tex)
    for g, w, t, h, what in zip(got, want, (want_rec, want_texels, R.pack(case.tris, mats, 1)[0]), (host[0], host[1], None), ("material records", "texels", "triangle records")):
        assert g == w, what + ": a context created from the same arrays"
        assert g == t.tobytes(), what + ": the numpy restatement"
        assert h is None or g == h.tobytes(), what + ": adypt_pack_appearance"
    after = p.ReadTriangleRecords()
    assert np.array_equal(after[:, :18], before[:, :18]) and np.array_equal(after[:, 20:], before[:, 20:]) and not np.array_equal(after[:, 19], before[:, 19])
    assert p.ReadTriangles().tobytes() == flat(case.tris).tobytes()
    p.destroy()


# ---- 2. the image equals the oracle bit for bit ----
def floor_attributes(case, mats):
    """the white triangles become `red`'s (textured in the new table) and get texture coordinates: (first, ids, texcoords, the new triangle array)"""
    old = np.array(case.scene.materials).view(O.MAT_DT)
    white, red = index_of(old, (0.75, 0.75, 0.75)), index_of(old, (0.75, 0.15, 0.15))
    idx = np.flatnonzero(case.tris["matid"] == white)
    first, count = int(idx[0]), int(idx[-1] - idx[0] + 1)
    t = case.tris.copy()
    sl = slice(first, first + count)
    t["matid"][sl] = np.where(t["matid"][sl] == white, red, t["matid"][sl])
    t["tc"][sl] = np.random.RandomState(4).uniform(-2, 2, size=t["tc"][sl].shape).astype(np.float32)
    return first, t["matid"][sl].copy(), t["tc"][sl].reshape(-1, 6).copy(), t


@pytest.mark.parametrize("name,variant", [("tiny0", "fused"), ("tiny0", "launch_per_bounce"), ("tiny0", "remap"), ("tiny0", "shade_bin"), ("tiny1", "fused"),
                                          ("tiny0", "attributes"), ("tiny0", "update_texture"), ("tiny0", "dark")])
def test_image_after_a_change(name, variant, scene_cache, sobol_matrices, monkeypatch):
    case = G.case_of(name, scene_cache)
    b = case.bvh(48)
    if name == "tiny1":
        assert len(b.tri_indices) > len(case.tris)  # references outnumber triangles: the per-reference copy is not the records
    if variant == "remap":
        monkeypatch.setenv("ADYPT_REF_TRIANGLES_MAX_MB", "0")
    if variant == "shade_bin":
        monkeypatch.setenv("ADYPT_SHADE_BIN", "1")
    mats, tex = new_table(case, glow=variant != "dark")  # (dark: the lamp off and nothing else on — a black image, which differs from the old one)
    tris = case.tris
    p = G.tracer(case, case.scene, b)
    if variant == "launch_per_bounce":
        p.SetFusedBounces(False)
    p.Trace(True, 2)  # (the old surfaces have been rendered: per-reference records, primary-hit cache and image are theirs)
    p.SetMaterials(mats, tex)
    if variant == "attributes":
        first, ids, uv, tris = floor_attributes(case, mats)
        p.Trace(True, 1)
        info = p.SetTriangleAttributes(first, ids, uv)
        assert info["reclassed"] > 0  # (glossy `white` -> diffuse `red`)
        assert p.ReadTriangles().tobytes() == flat(tris).tobytes()
    if variant == "update_texture":
        tex = [texture(5, 3, 41)]
        p.Trace(True, 1)
        assert p.UpdateTexture(0, tex[0])["reclassed"] == 0
        assert p.ReadTexels().tobytes() == A.arena(tex).tobytes()
    assert p.GetSPP() == 0
    p.Trace(True, SPP)
    assert p.GetFusedBounces() == (variant != "launch_per_bounce")
    plain = variant in ("fused", "launch_per_bounce", "remap", "shade_bin")
    want = oracle_image(case, 48, tris, mats, tex, sobol_matrices, key=(name, "new") if plain else None)
    assert np.array_equal(bits(p.ReadResult()), bits(want)), "the image of the new surfaces"
    assert want.any() == (variant != "dark")
    old = oracle_image(case, 48, case.tris, case.scene.materials, case.scene.textures, sobol_matrices, key=(name, "old"))
    assert not np.array_equal(bits(want), bits(old))  # the change shows
    if variant in ("attributes", "update_texture"):
        assert not np.array_equal(bits(want), bits(oracle_image(case, 48, case.tris, mats, new_table(case)[1], sobol_matrices, key=(name, "new"))))  # ... and so does the second one
    p.destroy()


# ---- 3. in the middle of an accumulation ----
@pytest.mark.parametrize("setting", ["frozen_blocks", "lookahead", "sun_query"])
def test_change_in_the_middle_of_an_accumulation(setting, scene_cache):
    case = G.case_of("tiny0", scene_cache)
    mats, tex = new_table(case)
    p = G.tracer(case, case.scene, case.bvh(48))
    if setting == "frozen_blocks":
        p.SetNoiseStats(True)
        r = p.TraceAdaptive(1e30, min_spp=2, max_spp=8, check_every=2)
        assert r["blocks_frozen"] == r["blocks"] > 0 and (p.ReadBlockSPP()[1] == 2).all()
    elif setting == "lookahead":
        p.SetFramesInFlight(4)
        p.SetLookahead(True)
        p.Trace(True, 1)
        assert p.GetLookaheadFrames() == 3
    else:
        p.SetSunVisibility(True, [0.6, 1.0, 0.2])
        p.Trace(True, 3)
    p.SetMaterials(mats, tex)
    assert p.GetSPP() == 0 and p.GetLookaheadFrames() == 0
    if setting == "lookahead":
        for _ in range(SPP):
            p.Trace(True, 1)
    else:
        p.Trace(True, SPP)
    assert p.GetSPP() == SPP
    if setting == "frozen_blocks":
        assert (p.ReadBlockSPP()[1] == SPP).all()  # thawed
    fresh = G.tracer(case, scene_of(case.tris, mats, tex), case.bvh(48))
    if setting == "sun_query":
        fresh.SetSunVisibility(True, [0.6, 1.0, 0.2])
    fresh.Trace(True, SPP)
    assert np.array_equal(bits(p.ReadResult()), bits(fresh.ReadResult())), setting
    fresh.destroy()
    p.destroy()


# ---- 4. the texel kernel at its edges ----
def test_texels_at_the_edges(scene_cache):
    case = G.case_of("tiny0", scene_cache)
    p = G.tracer(case, case.scene, case.bvh(48))
    tex = textures_of(SIZES)
    assert not np.array_equal(tex[8][0], tex[8][-1])  # first and last row differ: a wrap texel taken from another row shows
    mats = numbered_materials([-1, 0, len(tex) - 1, len(tex)])
    info = p.SetMaterials(mats, tex)
    assert info["n_textures"] == len(SIZES) and info["n_texels"] == sum((w + 1) * h for w, h in SIZES)
    assert p.ReadTexels().tobytes() == A.arena(tex).tobytes(), "every size in one call"
    assert p.ReadMaterialRecords().tobytes() == A.records(mats, tex).tobytes()
    for i, (w, h) in enumerate(SIZES):  # one at a time, in place: the others keep their words
        tex[i] = texture(w, h, 500 + i)
        p.UpdateTexture(i, tex[i])
        assert p.ReadTexels().tobytes() == A.arena(tex).tobytes(), (w, h)
    # the textures stay under a new table, and go with an empty list
    p.SetMaterials(mats[:2])
    assert p.ReadTexels().tobytes() == A.arena(tex).tobytes() and p.ReadMaterialRecords().tobytes() == A.records(mats[:2], tex).tobytes()
    info = p.SetMaterials(np.zeros(0, np.uint8), [])
    assert (info["n_mats"], info["n_textures"], info["n_texels"]) == (0, 0, 0) and p.ReadTexels().size == 0 and p.ReadMaterialRecords().shape == (0, 20)
    assert (p.ReadTriangleRecords()[:, 19] == 0).all()
    p.destroy()


# ---- 5. attribute ranges ----
def test_attribute_ranges(scene_cache):
    case = G.case_of("soup", scene_cache)
    n = len(case.tris)
    _, mats, _ = class_soup()  # eight materials in which every class occurs; its two "textures":
    tex = textures_of([(3, 1), (2, 1)])
    p = G.tracer(case, case.scene, case.bvh(48))
    p.SetMaterials(mats, tex)
    model = case.tris.copy()
    rs = np.random.RandomState(9)

    def held(what):
        assert p.ReadTriangleRecords().tobytes() == R.pack(model, mats, 2)[0].tobytes(), what

    def change(first, count, ids, uv):
        sl = slice(first, first + count)
        was = R.pack(model, mats, 2)[0][:, 19].copy()
        new_ids = rs.randint(-1, 10, size=count).astype(np.int32) if ids else None  # (-1, 8 and 9: no such material)
        new_uv = rs.uniform(-3, 3, size=(count, 6)).astype(np.float32) if uv else None
        if ids:
            model["matid"][sl] = new_ids
        if uv:
            model["tc"][sl] = new_uv.reshape(count, 3, 2)
        info = p.SetTriangleAttributes(first, new_ids, new_uv)
        assert info["reclassed"] == (R.pack(model, mats, 2)[0][:, 19] != was).sum(), (first, count)
        held((first, count, ids, uv))
    held("after SetMaterials")
    for first, count in ((0, 1), (255, 2), (4999, 1), (0, n)):
        change(first, count, True, True)
    change(100, 700, True, False)
    change(300, 513, False, True)
    assert set(np.unique(p.ReadTriangleRecords()[:, 19])) == {0, 1}
    p.destroy()


# ---- 6. refusals change nothing ----
def test_refusals_change_nothing(scene_cache, sobol_matrices):
    case = G.case_of("tiny0", scene_cache)
    mats, tex = new_table(case)
    n = len(case.tris)
    p = G.tracer(case, case.scene, case.bvh(48))
    p.SetMaterials(mats, tex)
    p.Trace(True, 2)
    before, c = state_of(p), p._ctx
    m, t = flat(mats), tex[0]
    arr = (N.Texture * 1)()
    ids, uv = np.zeros(n, np.int32), np.zeros((n, 6), np.float32)

    def set_materials(mp, n_mats, w, h, rgb, n_tex=1, table=True):
        arr[0].width, arr[0].height, arr[0].rgb = w, h, rgb
        return N.lib.adypt_set_materials(c, mp, n_mats, C.addressof(arr) if table else None, n_tex)
    calls = [
        lambda: set_materials(None, len(mats), 5, 3, t.ctypes.data),                # a null table
        lambda: set_materials(m.ctypes.data, -1, 5, 3, t.ctypes.data),              # n_mats < 0
        lambda: set_materials(m.ctypes.data, len(mats), 0, 3, t.ctypes.data),       # width <= 0
        lambda: set_materials(m.ctypes.data, len(mats), 5, -1, t.ctypes.data),      # height <= 0
        lambda: set_materials(m.ctypes.data, len(mats), 5, 3, None),                # null rgb
        lambda: set_materials(m.ctypes.data, len(mats), 2 ** 16, 2 ** 15, t.ctypes.data),  # 2^31 texels and more
        lambda: set_materials(m.ctypes.data, len(mats), 5, 3, t.ctypes.data, table=False),  # textures null with n_textures 1
        lambda: set_materials(m.ctypes.data, len(mats), 5, 3, t.ctypes.data, n_tex=-2),
        lambda: N.lib.adypt_update_texture(c, 1, t.ctypes.data, 5, 3),              # no such texture
        lambda: N.lib.adypt_update_texture(c, -1, t.ctypes.data, 5, 3),
        lambda: N.lib.adypt_update_texture(c, 0, None, 5, 3),
        lambda: N.lib.adypt_update_texture(c, 0, t.ctypes.data, 3, 5),              # another size
        lambda: N.lib.adypt_update_texture(c, 0, t.ctypes.data, 5, 4),
        lambda: N.lib.adypt_set_triangle_attributes(c, 0, n, None, None),           # both null
        lambda: N.lib.adypt_set_triangle_attributes(c, 1, n, ids.ctypes.data, None),
        lambda: N.lib.adypt_set_triangle_attributes(c, -1, 2, ids.ctypes.data, uv.ctypes.data),
        lambda: N.lib.adypt_set_triangle_attributes(c, n + 1, 0, None, uv.ctypes.data),
        lambda: N.lib.adypt_set_triangle_attributes(c, 0, -1, ids.ctypes.data, None),
    ]
    for k, call in enumerate(calls):
        assert call() == N.E_INVALID and N.lib.adypt_last_error(c), k
        assert p.GetSPP() == 2, k
    assert state_of(p) == before
    assert N.lib.adypt_read_material_records(c, None) == N.E_INVALID and N.lib.adypt_read_texels(c, None) == N.E_INVALID and N.lib.adypt_get_appearance(c, None) == N.E_INVALID
    with pytest.raises(ValueError):
        p.SetTriangleAttributes(0, ids[:3], uv[:4])
    with pytest.raises(N.AdyptError):
        p.UpdateTexture(0, texture(4, 3, 0))
    p.Trace(True, SPP - 2)  # the accumulation goes on
    assert np.array_equal(bits(p.ReadResult()), bits(oracle_image(case, 48, case.tris, mats, tex, sobol_matrices, key=("tiny0", "new"))))
    p.destroy()


# ---- 7. it stays out of the others' way ----
def test_geometry_calls_keep_the_attributes(scene_cache):
    case = G.case_of("tiny0", scene_cache)
    mats, tex = new_table(case)
    first, ids, uv, tris = floor_attributes(case, mats)
    n = len(tris)
    p = G.tracer(case, case.scene, case.bvh(48))
    p.BindParts(np.zeros(n, np.int32), 1)  # (bound before the attributes change)
    p.SetMaterials(mats, tex)
    p.SetTriangleAttributes(first, ids, uv)
    want = R.pack(tris, mats, 1)[0][:, 18:26]

    def kept(what):
        rec = p.ReadTriangleRecords()
        assert rec[:, 18:26].tobytes() == want.tobytes(), what
        return rec
    moved = G.pose(case.tris, True)
    G.update(p, moved, True)
    assert not np.array_equal(kept("UpdateTriangles")[:, :18], R.pack(tris, mats, 1)[0][:, :18])
    p.Pose(np.array([[1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, 0]], np.float32))
    kept("Pose")
    idx, pos, nrm = api.weld_triangles(flat(case.tris))
    p.BindMesh(idx, len(pos))
    p.PoseVertices(pos + np.float32(0.25), nrm)
    kept("PoseVertices")
    p.RebuildBVH(method="ploc")
    kept("RebuildBVH")
    # new triangles are packed with the table as it is now
    p.SetTriangles(flat(tris))
    assert p.ReadTriangleRecords().tobytes() == R.pack(tris, mats, 1)[0].tobytes(), "SetTriangles after SetMaterials"
    p.destroy()


def test_the_denoiser_history_survives(scene_cache):
    case = G.case_of("tiny0", scene_cache)
    old = np.array(case.scene.materials).view(O.MAT_DT)

    def run(change):
        p = G.tracer(case, case.scene, case.bvh(48))
        p.SetNoiseStats(True)
        p.Trace(True, SPP)
        p.Denoise(temporal=True)  # committed
        change(p)
        assert p.GetSPP() == 0
        p.Trace(True, SPP)
        out = p.Denoise(temporal=True, commit=False)
        n, hit = p.ReadDenoiseHistory(), p.ReadDenoiseGuides()["hit"]
        p.destroy()
        return out, n, hit
    # the unchanged table: the bits of a context that called Reset() instead
    a, b = run(lambda p: p.SetMaterials(old)), run(lambda p: p.Reset())
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert (b[1][b[2]] > np.float32(SPP)).any()  # (there was history to keep)
    # only the lamp's emission changes: no surface is repainted, the history is taken
    dim = old.copy()
    dim["ke"] *= np.float32(0.25)
    assert not np.array_equal(dim["ke"], old["ke"])
    out, n, hit = run(lambda p: p.SetMaterials(dim))
    assert hit.any() and (n[hit] > np.float32(SPP)).any()
    assert not np.array_equal(bits(out), bits(b[0]))


# ---- 8. several devices ----
def test_two_shards_on_one_device(scene_cache, monkeypatch):
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    case = G.case_of("tiny0", scene_cache)
    mats, tex = new_table(case)
    first, ids, uv, tris = floor_attributes(case, mats)
    w, h = 64, 36  # 2 x 2 blocks: both shards own some
    single = G.tracer(case, case.scene, case.bvh(48), w, h)
    multi = G.tracer(case, case.scene, case.bvh(48), w, h, cls=api.MultiPathTracer, devices=(0, 0))
    shards = [G.tracer(case, case.scene, case.bvh(48), w, h, tile_rank=r, tile_nranks=2) for r in range(2)]  # as one process per GPU makes them
    assert multi.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in multi._contexts())
    tex2 = [texture(5, 3, 77)]
    for t in [single, multi] + shards:
        t.Trace(True, 2)
        t.SetMaterials(mats, tex)
        t.SetTriangleAttributes(first, ids, uv)
        t.UpdateTexture(0, tex2[0])
        assert t.GetSPP() == 0
        t.Trace(True, SPP)
    want = state_of(single)
    assert want[1] == A.arena(tex2).tobytes() and want[2] == R.pack(tris, mats, 1)[0].tobytes()
    for c in multi._contexts():  # every device changed its own copy
        rec, texels, tr = np.zeros((len(mats), 20), np.uint32), np.zeros(18, np.uint32), np.zeros((len(tris), 32), np.uint32)
        N.check(N.lib.adypt_read_material_records(c, rec.ctypes.data), c)
        N.check(N.lib.adypt_read_texels(c, texels.ctypes.data), c)
        N.check(N.lib.adypt_read_triangle_records(c, tr.ctypes.data), c)
        assert (rec.tobytes(), texels.tobytes(), tr.tobytes()) == want
    image = single.ReadResult()
    assert np.array_equal(bits(multi.ReadResult()), bits(image))
    assert image.any()
    # the shards' own blocks are the single context's: block (bx, by) is rank (bx + by) % 2's, and a shard's read-out holds nothing else
    by, bx = np.mgrid[0:h, 0:w] // 32
    for r, s in enumerate(shards):
        assert state_of(s) == want
        part, owned = s.ReadResult(), (bx + by) % 2 == r
        assert np.array_equal(bits(part[owned]), bits(image[owned])) and not part[~owned].any(), r
    with pytest.raises(N.AdyptError) as e:
        multi.SetTriangleAttributes(1, np.zeros(len(tris), np.int32))
    assert e.value.code == N.E_INVALID
    for t in [single, multi] + shards:
        t.destroy()
