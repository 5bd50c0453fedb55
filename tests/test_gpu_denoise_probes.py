"""-m gpu: the denoiser's kernels (csrc/device/denoise_kernels.hpp, the header denoise.hip compiles) ONE BY ONE on the hand-made edge images of
tests/denoise_edge_inputs.py, through adypt_amd/libadypt_probe.so (tests/probe.py), which launches each kernel with the launch shape the product uses.
The render tests hold these kernels only at what two well-behaved scenes produce; here they see pictures smaller than a workgroup, a block and a halo,
block lists in any order, hit words that are no known triangle, NaN and Inf in every field, every refusal of a tap in turn, and reprojections a hair
outside the border.

Comparison: probe.same — equal bits, or NaN on both sides — against the stage-level numpy truths; no tolerance anywhere.  Every output is filled with a
sentinel word before the launch, and every pixel must have lost it.  Every case asserts, from its inputs or from the truth's side and never from the
device's output, that the branch it exists for is reached.  At the end the same small sizes go through the product's own calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api  # noqa: E402
from tests import denoise_edge_inputs as E  # noqa: E402
from tests import denoise_truth as D  # noqa: E402
from tests import probe as P  # noqa: E402
from tests import rectify_truth as R  # noqa: E402
from tests import temporal_motion_truth as TM  # noqa: E402
from tests import temporal_truth as TT  # noqa: E402
from tests.probe import same  # noqa: E402

F = np.float32
FILTER, TEMPORAL, RECTIFY, MOTION, GATHER = E.filter_cases(), E.temporal_cases(), E.rectify_cases(), E.motion_cases(), E.gather_cases()


def check(got, want, what):
    """probe.same everywhere and no word left unwritten; the message names the first mismatches."""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    left = P.unwritten(got)
    assert not left.any(), "%s: %d words were written by no thread, the first at %s" % (what, int(left.sum()), np.argwhere(left)[0].tolist())
    ok = same(got, want)
    if not ok.all():
        at = np.argwhere(~ok)[:6]
        lines = ["%s: device %r (%#x) truth %r (%#x)" % (i.tolist(), float(got[tuple(i)]), int(got.view(np.uint32)[tuple(i)]), float(want[tuple(i)]), int(want.view(np.uint32)[tuple(i)]))
                 for i in at]
        raise AssertionError("%s: %d of %d words differ\n%s" % (what, int((~ok).sum()), ok.size, "\n".join(lines)))


# ---- k_denoise_prepare ----
def _prepare_params():
    out = []
    for name, case in FILTER.items():
        h, w = case["call"][6].shape
        seen = []
        for order_name, order in E.block_orders(w, h).items():
            if tuple(order) not in seen:  # (a picture of one block has one order; of two, the rank-major order of 3 shards is the ascending one)
                seen.append(tuple(order))
                out.append(pytest.param(name, order_name, id="%s-%s" % (name, order_name)))
    return out


@pytest.mark.parametrize("name, order_name", _prepare_params())
def test_prepare(name, order_name):
    case = FILTER[name]
    assert case["reach"](), "the case does not reach what it is named after"
    call = case["call"]
    h, w = call[6].shape
    order = E.block_orders(w, h)[order_name]
    if order_name != "ascending":
        assert not np.array_equal(order, np.sort(order)), "the block list is the ascending one"
    inp = E.prepare_inputs(call, order, np.random.RandomState(7))
    words = E.hit_word_image(np.asarray(call[6]).astype(bool))
    if call[6].sum() >= len(E.HIT_WORDS):
        assert (words == -2).any() and (words == -7).any() and (words == 2 ** 31 - 1).any(), "no hit word that is neither -1 nor a known triangle"
    got = P.denoise_prepare(inp["accum"], inp["moments"], inp["albedo"], inp["normal"], inp["position"], inp["hits"], inp["blocks"], inp["block_spp"], w, h)
    for k, (g, t) in enumerate(zip(got, E.x_images(E.images(call)))):
        check(g, t, "%s, blocks %s: %s" % (name, order_name, ("X0", "X1", "X2", "XA")[k]))


# ---- k_atrous ----
def _atrous_params():
    out = [pytest.param(name, step, s, last, id="%s-step%d-sigmas%d-%s" % (name, step, s, "last" if last else "level"))
           for name in ("rough-33x9", "rough-70x40") for step in E.STEPS for s in (0, 1) for last in (False, True)]
    return out + [pytest.param(name, 1, 0, last, id="%s-step1-sigmas0-%s" % (name, "last" if last else "level")) for name in FILTER if name not in ("rough-33x9", "rough-70x40")
                  for last in (False, True)]


@pytest.mark.parametrize("name, step, sigmas, last", _atrous_params())
def test_atrous(name, step, sigmas, last):
    case = FILTER[name]
    assert case["reach"](), "the case does not reach what it is named after"
    im = E.images(case["call"])
    h, w = im["hit"].shape
    assert step == 1 or step < w, "no tap of this step lies inside the picture"
    sigma_l, sigma_z = E.SIGMAS[sigmas]
    D1, V1 = D.level(im["D"], im["V"], im["N"], im["P"], im["hit"], step, sigma_l, sigma_z)
    if last:
        assert w == 1 or (im["A"][:, 1:] != im["A"][:, :-1]).any() or not im["hit"].any(), "the albedo is flat: a neighbour's would do"
        with np.errstate(all="ignore"):
            want = D1 * im["ka"]
    else:
        want = E.rgba(D1, V1)
    check(P.atrous(*E.x_images(im), step, sigma_l, sigma_z, last), want, "%s, step %d, sigmas %s, last %s" % (name, step, (sigma_l, sigma_z), last))


# ---- k_rectify_window ----
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("name", list(RECTIFY))
def test_window(name, radius):
    case = RECTIFY[name]
    assert case["reach"](E.rectify_truth(case)), "the case does not reach what it is named after"
    im = E.images(case["call"])
    assert im["hit"].any()
    R0, R1 = R.window(im["D"], im["V"], im["N"], im["P"], im["A"], im["hit"], case["cam"][0], radius)
    g0, g1 = P.rectify_window(radius, *E.x_images(im), case["cam"][0])
    check(g0, R0, "%s, radius %d: R0" % (name, radius))
    check(g1, R1, "%s, radius %d: R1" % (name, radius))


# ---- k_temporal_merge, all four instances ----
HOME = {}  # case id -> (the case, the truth its reach is asked of)
for _name, _case in TEMPORAL.items():
    HOME["temporal/" + _name] = (_case, E.merge_truth)
for _name, _case in RECTIFY.items():
    HOME["rectify/" + _name] = (_case, E.rectify_truth)
for _name, _case in MOTION.items():
    HOME["motion/" + _name] = (_case, E.motion_truth)


@pytest.mark.parametrize("motion, rectify", [(False, False), (True, False), (False, True), (True, True)], ids=["plain", "motion", "rectified", "motion-rectified"])
@pytest.mark.parametrize("key", list(HOME))
def test_merge(key, motion, rectify):
    case, home_truth = HOME[key]
    assert case["reach"](home_truth(case)), "the case does not reach what it is named after"
    kw = case["kw"]
    cap, radius, gamma = kw.get("cap", 64.0), kw.get("radius", 3), kw.get("gamma", 1.0)
    im = E.images(case["call"])
    h, w = im["hit"].shape
    hist = case["hist"]
    # where the pixel's surface was: the motion cases' triangles say; every other case stands still (XP = P, not moved; XN = N, valid)
    if "tri" in case:
        Pp, moved, Np, valid = TM.previous_point(None if hist is None else hist.get("tris"), case["cur"], case["tri"], case["uv"], im["N"], im["P"])
    else:
        Pp, moved, Np, valid = im["P"], np.zeros((h, w), bool), im["N"], np.ones((h, w), bool)
    XP, XN = E.rgba(Pp, moved.astype(np.float32)), E.rgba(Np, valid.astype(np.float32))
    R0 = R1 = kept = None
    if rectify:
        R0, R1 = R.window(im["D"], im["V"], im["N"], im["P"], im["A"], im["hit"], case["cam"][0], radius)
        Dm, Vm, no, kept = R.merge(im["D"], im["V"], im["n"], im["N"], im["P"], im["A"], im["hit"], hist, R0, R1, gamma, cap, through=(Np, Pp, valid) if motion else None)
    elif motion:
        Dm, Vm, no = TT.merge(im["D"], im["V"], im["n"], Np, Pp, im["A"], im["hit"] & valid, hist, cap)
    else:
        Dm, Vm, no = TT.merge(im["D"], im["V"], im["n"], im["N"], im["P"], im["A"], im["hit"], hist, cap)
    # (a call without a history is given what lies in the history's memory all the same — "stale", as after a reset — and told that there is none)
    H, raw = E.h_images(hist if hist is not None else case.get("stale"), h, w)
    got = P.temporal_merge(E.x_images(im), H, hist is not None, raw, cap, motion=(XP, XN) if motion else None, rectify=(R0, R1, gamma) if rectify else None)
    what = "%s, motion %s, rectify %s: " % (key, motion, rectify)
    check(got[0], E.rgba(Dm, Vm), what + "the merged image")
    check(got[1], E.rgba(im["P"], no), what + "X2 with n_out")
    check(got[2], no, what + "the history length")
    if rectify:
        check(got[3], kept, what + "kept")


# ---- k_motion_gather ----
def _gather_params():
    out = []
    for name, case in GATHER.items():
        seen = []
        for order_name, order in E.block_orders(case["w"], case["h"]).items():
            if tuple(order) not in seen:
                seen.append(tuple(order))
                out.append(pytest.param(name, order_name, id="%s-%s" % (name, order_name)))
    return out


@pytest.mark.parametrize("name, order_name", _gather_params())
def test_gather(name, order_name):
    case = GATHER[name]
    w, h, tri, n_known = case["w"], case["h"], case["tri"], case["n_known"]
    XP, XN, moved, valid = E.gather_truth(case)
    # what the case is for, from its inputs and the truth: never an index farther than 32 from either end of [0, n_known)
    assert tri.min() >= -32 and tri.max() < n_known + 32
    present = [int(v) for v in E.gather_words(n_known) if (tri == v).any()]
    assert w * h < 12 or present == [int(v) for v in E.gather_words(n_known)], "a hit word is missing: %s" % present
    if n_known == 0:
        assert not moved.any() and (tri == 0).any() and (tri == 5).any()
    elif w * h >= 12:
        assert not moved[tri == 0].any() and moved[tri == 1].all(), "18 equal words are unmoved, one differing bit in word 17 is moved"
        assert (tri == n_known - 1).any() and moved[tri == n_known - 1].all() and not moved[(tri < 0) | (tri >= n_known)].any()
        assert not valid[tri == 3].any() and not valid[tri == 4].any() and valid[tri == 2].all(), "previous normals that sum to 0, or hold Inf, are not valid"
        uv = case["uv"][tri == 2]
        assert all((uv == F(c)).all(-1).any() for c in ([0, 0], [1, 0], [0, 1], [0.5, 0.5])), "u, v at 0, 1 and (0.5, 0.5) on a moved triangle"
    order = E.block_orders(w, h)[order_name]
    inp = E.gather_inputs(case, order)
    gp, gn = P.motion_gather(inp["hits"], inp["normal"], inp["position"], order, w, h, case["snapshot"], case["records"])
    check(gp, XP, "%s, blocks %s: XP" % (name, order_name))
    check(gn, XN, "%s, blocks %s: XN" % (name, order_name))
    for g in (gp, gn):
        assert not (g == E.SLACK_VALUE).any() and not (g == E.POISON).any(), "a word from outside the tables, or from beyond word 19 of a record"


# ---- k_motion_snapshot ----
@pytest.mark.parametrize("n", E.SNAPSHOT_COUNTS)
def test_snapshot(n):
    records = E.snapshot_records(n)
    assert records.shape == (n, 32) and (records[:, 20:] == E.POISON).all() and not (records[:, :20] == E.POISON).any()
    got = P.motion_snapshot(records)
    check(got, records[:, :20], "%d triangles" % n)
    assert not (got == E.POISON).any(), "a word from beyond the first 80 bytes of a record"


# ---- the same sizes through the product ----
@pytest.mark.parametrize("size", [(1, 1), (3, 2), (31, 7)], ids=["1x1", "3x2", "31x7"])
def test_small_pictures_through_the_product(size, scene_cache, sobol_matrices):
    """tiny0 smaller than one workgroup, one block and one halo: Denoise(), two temporal calls with the camera unchanged, one rectified call at radius 3
    (following motion and committing, so that it leaves a snapshot) and one follow_motion call after a Pose that turns the box, each against the truth of
    the oracle's images.  The config's camera gives hit pixels at 3x2 and 31x7 (asserted from the oracle's guides)."""
    from oracle import oracle_py as O
    from tests import rectify_truth as RT
    from tests import test_gpu_denoise_motion as M
    from tests import test_gpu_denoise_temporal as TG
    from tests.helpers import oracle_scene_from_instance
    w, h = size
    inst, _, tris, on_box = M.instance(scene_cache, w, h)
    p, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    pos, yaw = TG.camera_of(c, "tiny0", 0)

    def pose(key, osc, seed):
        call, cam, _, tri = TG.oracle_pose(("small", w, h, key), osc, c, pos, yaw, seed, sobol_matrices)
        ip, iv = O.camera(c.fov, yaw, c.pitch, w, h)
        prm = O.make_params(w, h, pos, ip, iv, stack_size=c.stack_size, max_bounce=c.max_bounce, subpixel=c.subpixel, tmp_life=c.tmp_lifetime, tmin=c.ray_tmin, clamp=c.clamp,
                            sun=list(c.sun))
        hits = O.primary_frame(osc, prm, 0)[1]
        assert np.array_equal(hits["tri_id"], tri)
        return call, cam, tri, np.stack([hits["u"], hits["v"]], -1).astype(np.float32)
    call, cam, tri, uv = pose("rest", oracle_scene_from_instance(inst), TG.SEED)
    print("tiny0 %dx%d: %d of %d pixels hit" % (w, h, int(call[6].sum()), w * h))
    if size != (1, 1):
        assert call[6].any(), "the config's camera sees nothing at this size"
    TG.set_pose(p, cfg, pos, yaw, TG.SEED)
    assert TG.same(p.ReadResult(), call[0]), "the image is not the oracle's"
    assert TG.same(p.Denoise(), D.denoise(*call)), "Denoise()"
    hist = None
    for k in range(2):
        want, want_n, hist = TT.denoise(*call, hist, cam)
        assert TG.same(p.Denoise(temporal=True), want) and TG.same(p.ReadDenoiseHistory(), want_n), "temporal call %d" % k
    if call[6].any():
        assert (want_n[call[6]] > F(TG.SPP)).any(), "no pixel found its own history under an unchanged camera"
    want, want_n, hist, extra = RT.denoise(*call, hist, cam, radius=3, motion=(tri, uv, M.words(tris)))
    got = p.Denoise(temporal=True, rectify=True, rectify_radius=3, follow_motion=True)
    assert TG.same(got, want) and TG.same(p.ReadDenoiseHistory(), want_n) and TG.same(p.ReadDenoiseRectify(), extra["kept"]), "the rectified call"
    assert p.GetDenoiseMotion()["have_snapshot"] == 1
    # the box turned by a Pose, the camera where it was
    parts, matrices = M.rotation_matrices(tris, on_box)
    turned = np.array(api.pose_triangles(tris, matrices, parts=parts)).view(O.TRI_DT)
    b = api.WideBVH()
    b.BuildPLOC(api.Scene.FromArrays(turned, inst.scene.materials), cfg.bvh_params(), 8, 0.0)
    osc = O.Scene(b.nodes, b.tri_indices, np.ascontiguousarray(turned).view(np.uint8).reshape(-1), inst.scene.materials, textures=inst.scene.textures)
    call, cam, tri, uv = pose("turned", osc, TG.SEED + 1)
    p.BindParts(parts, 2)
    p.Pose(matrices)
    TG.set_pose(p, cfg, pos, yaw, TG.SEED + 1)
    assert TG.same(p.ReadResult(), call[0]), "the image of the turned box is not the oracle's"
    want, want_n, _, motion = TM.denoise(*call, hist, cam, tri, uv, M.words(turned))
    print("tiny0 %dx%d after the Pose: %d pixels on a moved triangle" % (w, h, int(motion["moved"].sum())))
    got = p.Denoise(temporal=True, follow_motion=True)
    read = p.ReadDenoiseMotion()
    assert TG.same(got, want) and TG.same(p.ReadDenoiseHistory(), want_n), "the follow_motion call after the Pose"
    assert TG.same(read["previous_position"], motion["previous_position"]) and np.array_equal(read["moved"], motion["moved"])
    p.destroy()
