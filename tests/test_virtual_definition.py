"""The temporal merge by the virtual point (csrc/device/guide_chain.hpp: the unfolded length and the virtual point; csrc/device/temporal.hpp:
temporal_merge_virtual) compiled on the host and held bit for bit against its numpy float32 restatement (tests/virtual_truth.py) over what the CPU oracle
gives; what can be derived of the planar scene is derived; the quality is measured against the oracle's converged image, never against the code under
test.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import denoise_truth as D
from tests import specular_truth as S
from tests import temporal_truth as TT
from tests import test_specular_definition as SD  # its driver source and its HeaderOps: the chain's operations through the compiled header
from tests import virtual_edge_inputs as E
from tests import virtual_scenes as VS
from tests import virtual_truth as V
from tests.denoise_edge_inputs import rgba
from tests.helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")
F = np.float32
SEED = 31

DRIVER = SD.DRIVER + r"""
struct VHist {
	const Dn4 *a, *b, *c, *d;
	Dn4 h0(int i) const { return a[i]; }
	Dn4 h1(int i) const { return b[i]; }
	Dn4 h2(int i) const { return c[i]; }
	Dn4 ha(int i) const { return d[i]; }
};
extern "C" {
void vp_start_length(int n, const float *p0, const float *origin, float *out) { for(int i = 0; i < n; ++i) out[i] = chain_start_length(ld(p0, i), origin); }
void vp_unfold(int n, const float *len, const float *hit, const float *ro, float *out) { for(int i = 0; i < n; ++i) out[i] = chain_unfold(len[i], ld(hit, i), ld(ro, i)); }
void vp_virtual_point(int n, const float *p0, const float *origin, const float *len, float *pv, uint8_t *valid)
{
	for(int i = 0; i < n; ++i)
	{
		const ChainVirtual v = chain_virtual_point(ld(p0, i), origin, len[i]);
		st(pv, i, v.p); valid[i] = v.valid ? 1 : 0;
	}
}
// cam: origin 3, inv_proj 16, inv_view 16; every image w x h Dn4; out: merged (w x h Dn4), n_out and kept (w x h floats)
void vp_merge(int w, int h, int have, const float *cam, float cap, const Dn4 *x0, const Dn4 *x1, const Dn4 *x2, const Dn4 *xa, const Dn4 *xv, const Dn4 *h0, const Dn4 *h1, const Dn4 *h2,
              const Dn4 *ha, Dn4 *merged, float *n_out, float *kept)
{
	const TemporalCamera tc = temporal_camera(cam, cam + 3, cam + 19);
	const VHist hist{h0, h1, h2, ha};
	for(int i = 0; i < w * h; ++i)
	{
		const TemporalOut m = temporal_merge_virtual(hist, have != 0, tc, w, h, x0[i], x1[i], x2[i], xa[i], xv[i], x2[i].w, cap);
		merged[i] = m.x0; n_out[i] = m.n; kept[i] = m.kept;
	}
}
}
"""

f32, ptr = SD.f32, SD.ptr


class HeaderUnfold:
    """virtual_truth.NumpyUnfold's operations through the compiled header."""

    def __init__(self, lib):
        self.lib = lib

    def start_length(self, p0, origin):
        p0, origin, out = f32(p0), f32(origin), np.zeros(len(p0), np.float32)
        self.lib.vp_start_length(len(p0), ptr(p0), ptr(origin), ptr(out))
        return out

    def unfold(self, length, hit, ray_origin):
        length, hit, ray_origin, out = f32(length), f32(hit), f32(ray_origin), np.zeros(len(hit), np.float32)
        self.lib.vp_unfold(len(hit), ptr(length), ptr(hit), ptr(ray_origin), ptr(out))
        return out

    def virtual_point(self, p0, origin, length):
        p0, origin, length = f32(p0), f32(origin), f32(length)
        pv, valid = np.zeros((len(p0), 3), np.float32), np.zeros(len(p0), np.uint8)
        self.lib.vp_virtual_point(len(p0), ptr(p0), ptr(origin), ptr(length), ptr(pv), ptr(valid))
        return pv, valid.astype(bool)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("virtual_driver")
    src, so = str(d / "driver.cpp"), str(d / "libdriver.so")
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", DEVICE, src, "-o", so])
    return C.CDLL(so)


def header_merge(lib, case):
    """vp_merge over raw images (tests/virtual_edge_inputs.py's layout): (Dm, Vm, n_out, kept)"""
    w, h = case["w"], case["h"]
    cam = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in case["cam"]])
    imgs = [f32(case[k]) for k in ("x0", "x1", "x2", "xa", "xv", "h0", "h1", "h2", "ha")]
    merged, n_out, kept = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    lib.vp_merge(w, h, int(case["have"]), ptr(cam), C.c_float(case["cap"]), *[ptr(a) for a in imgs], ptr(merged), ptr(n_out), ptr(kept))
    return merged[..., :3], merged[..., 3], n_out, kept


def raw_case(pose, g, hist, cam_of_hist, cap=64.0):
    """the raw images of a call with the oracle's pose and the guides g against the history `hist` (what V.commit made, or None)"""
    h, w = pose["m2"].shape
    n = D.block_counts(h, w, pose["spp"])
    D0, V0, _ = D.prepare(pose["image"], pose["m2"], n, g["albedo"])
    case = dict(w=w, h=h, cap=cap, have=0 if hist is None else 1, cam=cam_of_hist if hist is not None else (np.zeros(3, np.float32), np.zeros(16, np.float32), np.zeros(16, np.float32)),
                x0=rgba(D0, V0), x1=rgba(g["normal"], g["chain"].astype(np.float32)), x2=rgba(g["position"], n), xa=rgba(g["albedo"], 0.0), xv=rgba(g["virtual"], g["distance"]))
    z = np.zeros((h, w, 4), np.float32)
    case.update(dict(h0=z, h1=z, h2=z, ha=z) if hist is None else dict(h0=rgba(hist["D"], hist["V"]), h1=rgba(hist["N"], hist["cls"]), h2=rgba(hist["P"], hist["n"]), ha=rgba(hist["A"], 0.0)))
    return case


def differing(a, b):
    return int((bits(a) != bits(b)).sum())


def assert_merge(lib, case, tag):
    """the header's merge of a raw case against numpy's: zero differing words, `kept` untouched; returns numpy's n_out"""
    Dm, Vm, no, followed, with_history = E.truth(case)
    gD, gV, gn, kept = header_merge(lib, case)
    for name, got, want in (("merged D", gD, Dm), ("merged V", gV, Vm), ("n_out", gn, no)):
        assert differing(got, want) == 0, "%s: %d words of %s differ from the numpy restatement" % (tag, differing(got, want), name)
    assert (kept == F(1.0)).all(), tag + ": kept"
    return no


def assert_unfolded(got, want, tag):
    SD.assert_same_chain(got, want, tag)
    for k in ("length", "virtual", "distance"):
        assert differing(got[k], want[k]) == 0, "%s: %d words of %s differ from the numpy restatement" % (tag, differing(got[k], want[k]), k)


# ---- poses, once per session ----
_poses = {}


def tiny0_pose(scene_cache, sobol_matrices, k, spp=4, ref_spp=0):
    key = ("tiny0", k, spp, ref_spp)
    if key not in _poses:
        entry = VS.tiny0(scene_cache)
        P, cam = VS.tiny0_camera(entry, k)
        pose = VS.oracle_pose(entry[0], P, SEED + k, sobol_matrices, spp, ref_spp=ref_spp)
        pose.update(osc=entry[0], P=P, cam=cam)
        _poses[key] = pose
    return _poses[key]


def planar_pose(sobol_matrices, k, spp, w=45, h=21, ref_spp=0):
    key = ("planar", w, h, k, spp, ref_spp)
    if key not in _poses:
        b = _poses.setdefault(("planar", w, h), VS.Planar(w, h))
        osc, P = b.oracle_at(k)
        pose = VS.oracle_pose(osc, P, SEED + k, sobol_matrices, spp, ref_spp=ref_spp)
        pose.update(osc=osc, P=P, cam=b.camera(k), built=b)
        _poses[key] = pose
    return _poses[key]


def guides(pose, K):
    key = ("guides", K)
    if key not in pose:
        pose[key] = V.chain_guides(pose["osc"], pose["P"], K, pose["primary"])
    return pose[key]


def call_of(pose, g, hist, K, **kw):
    return V.denoise(pose["image"], pose["m2"], pose["spp"], g, hist, pose["cam"], K, **kw)


# ---- 1. the definition against the truth ----
def test_tiny0_lengths_virtual_points_and_merge(lib, scene_cache, sobol_matrices):
    """tiny0 100x75 at K = 1, 2, 8, two cameras a step apart: the header's chain with the length beside it, its virtual points and its merge against
    numpy, zero differing words; the guides beside them are tests/specular_truth.py's."""
    ops, unfold = SD.HeaderOps(lib), HeaderUnfold(lib)
    a, b = (tiny0_pose(scene_cache, sobol_matrices, k) for k in (0, 1))
    for K in (1, 2, 8):
        ga, gb = guides(a, K), guides(b, K)
        SD.assert_same_chain(ga, S.chain_guides(a["osc"], a["P"], K, a["primary"]), "the guides beside the length, K = %d" % K)
        assert_unfolded(V.chain_guides(b["osc"], b["P"], K, b["primary"], ops=ops, unfold=unfold), gb, "tiny0 K = %d" % K)
        followed = gb["chain"] >= 2
        assert followed.any() and (gb["distance"][followed] > 0).all() and (gb["distance"][~followed] == 0).all()
        assert np.array_equal(bits(gb["virtual"][~followed]), bits(gb["position"][~followed]))
        _, _, hist, _ = call_of(a, ga, None, K)
        no = assert_merge(lib, raw_case(b, gb, hist, a["cam"]), "tiny0 K = %d" % K)
        n = F(b["spp"])
        assert (no[followed] > n).any() and (no[gb["chain"] == 1] > n).mean() > 0.5 and (no[gb["chain"] <= 0] == n).all()


def test_planar_scene_is_bit_exact_and_its_geometry_is_the_derived_one(lib, sobol_matrices):
    """45 x 21 (neither a multiple of 32 wide nor of 8 high), the second camera 0.15 to the side and 1.5 degrees of yaw away, 2 spp each.

    The virtual point against the fp64 mirror image M(Ph) of the followed point Ph.  With u = 2^-24, len the unfolded length and V the largest
    vertex coordinate of the scene (the quads are 50 units wide: a hit point is an interpolation of vertices of that size), the bound is
        |Pv - M(Ph)| <= u (20 len + 36 V)
    from: (a) the four operations of the definition — e = P0 - O and len = sqrt(e . e) + sqrt(D . D) (each square root of a dot product 3.5 u
    relative, the sum 1 u: 4 u len), d0 = e / |e| (3 u as a direction), Pv = O + d0 len (2 u len): 9 u len in all; (b) the direction the oracle
    traced, which the truth's mirror arithmetic made from d0: k = 2 d . n (3 u), d - k n (2 u per term), on top of d0's 3 u: 8 u as a direction, so the
    followed point lies up to 8 u len beside the exact reflection — with (a) 17 u len, taken as 20; (c) what the points themselves carry: P0 and
    Ph are each (p0 u + p1 v) + p2 w with w = (1 - u) - v, five roundings of terms up to V: 5 u V per component, 8.7 u V as a vector, for both
    17.4 u V; and the barycentrics the intersection gave are themselves good to a few u of a triangle 2 V wide: 8 u . 2 V.  33.4 u V, taken as 36.

    Every pixel whose virtual point reprojects inside [0, W - 1] x [0, H - 1] has n_out == 4 exactly: its four taps are the same wall, each of
    length 2, and sum(w 2) / sum(w) is exactly 2."""
    a, b = (planar_pose(sobol_matrices, k, 2) for k in (0, 1))
    built = a["built"]
    ops, unfold = SD.HeaderOps(lib), HeaderUnfold(lib)
    for K in (1, 8):
        ga, gb = guides(a, K), guides(b, K)
        assert (gb["chain"] == 2).all() and (gb["distance"] > 0).all(), "every pixel sees the wall in the mirror"
        assert_unfolded(V.chain_guides(b["osc"], b["P"], K, b["primary"], ops=ops, unfold=unfold), gb, "planar K = %d" % K)
        want = built.mirror_image(gb["position"])
        err = np.sqrt(((gb["virtual"].astype(np.float64) - want) ** 2).sum(-1))
        u, vmax = 2.0 ** -24, float(np.abs(built.tris["p"]).max())
        bound = u * (20.0 * gb["distance"].astype(np.float64) + 36.0 * vmax)
        print("planar K = %d: |Pv - mirror image| at most %.3g, %.3f of the bound; len %.3f .. %.3f" % (K, err.max(), (err / bound).max(), gb["distance"].min(), gb["distance"].max()))
        assert (err <= bound).all()
        _, n_a, hist, _ = call_of(a, ga, None, K)
        assert (n_a == F(2)).all()
        no = assert_merge(lib, raw_case(b, gb, hist, a["cam"]), "planar K = %d" % K)
        ok, fx, fy, _ = TT.reproject(hist["cam"], 45, 21, gb["virtual"])
        inside = ok & (fx >= 0) & (fx <= F(44)) & (fy >= 0) & (fy <= F(20))
        assert inside.sum() > 45 * 21 // 2, "the second camera sees mostly what the first saw"
        assert (no[inside] == F(4)).all(), "%d pixels aimed inside the history are not of length 4" % int((no[inside] != F(4)).sum())
        # (for the record: where the same pixels land through the mirror's own surface, which is what the plain temporal call reprojects)
        _, sx, sy, _ = TT.reproject(hist["cam"], 45, 21, b["primary"]["position"])
        print("planar K = %d: through the mirror's surface the history is fetched up to %.2f px beside the virtual point's place" % (K, float(np.abs(sx - fx)[inside].max())))


def test_hand_made_edge_inputs(lib):
    """a tap off each image edge, a tap of another class, a NaN and an infinity in a tap, a length that is not valid: each entry reaches what it is
    named after by the truth's account, and the header's words are numpy's"""
    for name, case in E.cases().items():
        no = assert_merge(lib, case, name)
        assert case["reach"](no), name + ": the case does not reach what it is named after"


def test_lengths_that_overflow_and_a_primary_hit_at_the_camera(lib):
    ops, N = HeaderUnfold(lib), V.NumpyUnfold()
    o = f32([1.0, 2.0, 3.0])
    # len overflowing to an infinity: a ray 2e19 long in every component has a squared length beyond binary32
    hit, ro, ln = f32([[2e19, 2e19, 2e19], [3.0, 4.0, 0.0]]), f32([[0, 0, 0], [0, 0, 0]]), f32([5.0, 3.2e38])
    got, want = ops.unfold(ln, hit, ro), N.unfold(ln, hit, ro)
    assert differing(got, want) == 0 and np.isinf(got[0]) and got[1] == F(3.2e38), "an infinity, and a finite length beyond kTemporalFiniteMax"
    p0 = f32([[4.0, 6.0, 3.0], [4.0, 6.0, 3.0]])
    (pv, valid), (pw, vw) = ops.virtual_point(p0, o, got), N.virtual_point(p0, o, want)
    assert differing(pv, pw) == 0 and not valid.any() and not vw.any()
    # P0 at the camera origin: length 0, no direction, not valid — and the chain does not start there
    p0 = f32([o, o + f32([0, 0, 2.0])])
    ln = ops.start_length(p0, o)
    assert differing(ln, N.start_length(p0, o)) == 0 and ln[0] == 0 and ln[1] == F(2.0)
    (pv, valid), (pw, vw) = ops.virtual_point(p0, o, ln), N.virtual_point(p0, o, ln)
    assert differing(pv, pw) == 0 and list(valid) == [False, True] and list(vw) == [False, True]
    assert np.array_equal(pv[0], o) and np.array_equal(pv[1], p0[1])
    mirror = (np.array([False]), np.array([3], np.int32), f32([[0.9, 0.9, 0.9]]), f32([1.0]), f32([[0, 0, -1]]))
    for chain_ops in (SD.HeaderOps(lib), S.NumpyOps()):
        assert not chain_ops.at_primary(*mirror, p0[:1], o, 8)[0][0] and chain_ops.at_primary(*mirror, p0[1:], o, 8)[0][0]
    # a NaN length is refused
    (pv, valid) = ops.virtual_point(p0, o, f32([np.nan, np.nan]))
    assert not valid.any() and not N.virtual_point(p0, o, f32([np.nan, np.nan]))[1].any()


# ---- 3. identities ----
def test_without_delta_materials_it_is_the_plain_temporal_merge(scene_cache, sobol_matrices):
    """a tiny0 whose delta materials are made diffuse: classes 0 and 1 only, and the followed temporal truth is tests/temporal_truth.py's to the bit"""
    from oracle import oracle_py as O
    entry = VS.tiny0(scene_cache)
    osc = entry[0]
    mats = np.array(osc.materials).copy()
    assert np.isin(mats["illum"], (3, 4, 5, 6, 7)).any()
    mats["illum"][np.isin(mats["illum"], (3, 4, 5, 6, 7))] = 1
    matte = O.Scene(osc.nodes, osc.tri_indices, osc.triangles, mats, textures=osc.textures)
    hist_v = hist_t = None
    for k in (0, 1):
        P, cam = VS.tiny0_camera(entry, k)
        pose = VS.oracle_pose(matte, P, SEED + k, sobol_matrices, 4)
        g = V.chain_guides(matte, P, 8, pose["primary"])
        assert set(np.unique(g["chain"])) == {0, 1} and g["followed"] == 0
        out, no, hist_v, counts = V.denoise(pose["image"], pose["m2"], 4, g, hist_v, cam, 8)
        want, want_n, hist_t = TT.denoise(pose["image"], pose["m2"], 4, g["albedo"], g["normal"], g["position"], g["hit"], hist_t, cam)
        assert differing(out, want) == 0 and differing(no, want_n) == 0 and counts == dict(followed=0, with_history=0)
        for key in ("D", "V", "n"):
            assert differing(hist_v[key], hist_t[key]) == 0
    assert (no[g["hit"]] > F(4)).mean() > 0.5


def test_without_history_it_is_the_followed_filter_and_other_kinds_are_none(scene_cache, sobol_matrices):
    a, b = (tiny0_pose(scene_cache, sobol_matrices, k) for k in (0, 1))
    ga, gb = guides(a, 8), guides(b, 8)
    out, no, hist8, _ = call_of(a, ga, None, 8)
    assert differing(out, S.denoise(a["image"], a["m2"], a["spp"], ga["albedo"], ga["normal"], ga["position"], ga["chain"])) == 0 and (no == F(4)).all()
    none = call_of(b, gb, None, 8)
    with8 = call_of(b, gb, hist8, 8)
    assert differing(with8[0], none[0]) != 0 and (with8[1] > none[1]).any()
    # a history of another K, and a plain temporal call's: the same as none
    _, _, hist2, _ = call_of(a, guides(a, 2), None, 2)
    plain = TT.denoise(a["image"], a["m2"], a["spp"], a["primary"]["albedo"], a["primary"]["normal"], a["primary"]["position"], a["primary"]["tri"] != -1, None, a["cam"])[2]
    for other in (hist2, plain):
        got = call_of(b, gb, other, 8)
        assert differing(got[0], none[0]) == 0 and differing(got[1], none[1]) == 0
        for key in ("D", "V", "n"):
            assert differing(got[2][key], none[2][key]) == 0


# ---- 4. quality ----
def sequence_quality(name, poses, K=8, cap=64.0):
    """four cameras, committing; at the last: rmse of the followed spatial filter on its own 4 spp and of the followed temporal result against the
    oracle's converged image, over all pixels, the chain pixels (class != the primary hit flag) and the others"""
    hist = None
    for pose in poses:
        g = guides(pose, K)
        out, n_out, hist, counts = call_of(pose, g, hist, K, cap=cap)
    last, ref = poses[-1], poses[-1]["ref"]
    spatial = S.denoise(last["image"], last["m2"], last["spp"], g["albedo"], g["normal"], g["position"], g["chain"])
    chain_px = g["chain"].astype(np.int32) != (last["primary"]["tri"] != -1).astype(np.int32)
    followed = g["chain"] >= 2
    fig = {}
    for key, sel in (("all", np.ones_like(followed)), ("chain", chain_px), ("followed", followed), ("other", ~chain_px)):
        fig[key] = (D.rmse(spatial[sel], ref[sel]), D.rmse(out[sel], ref[sel])) if sel.any() else (0.0, 0.0)
    fig["share"] = counts["with_history"] / max(counts["followed"], 1)
    print("%s, 4 cameras x 4 spp, K = %d, cap %g, %d followed px (%.1f %% found history): rmse followed spatial -> followed temporal: all %.4f -> %.4f, chain px %.4f -> %.4f, "
          "followed px %.4f -> %.4f, other px %.4f -> %.4f" % ((name, K, cap, counts["followed"], 100.0 * fig["share"]) + fig["all"] + fig["chain"] + fig["followed"] + fig["other"]))
    return fig


def test_quality_planar(sobol_matrices):
    """the planar scene 45 x 21, four cameras a step apart, 4 spp each, against the oracle's 1024-spp image at the last: the followed temporal result has
    the lower error over all pixels and over the followed pixels (which are all of them).  Measured, printed here, quoted in DESIGN.md section 4,
    "Temporal merge through mirrors and glass" (rmse followed spatial -> followed temporal): 0.0696 -> 0.0556, 97.8 % of the 945 followed pixels found history."""
    poses = [planar_pose(sobol_matrices, k, 4, ref_spp=1024 if k == 3 else 0) for k in range(4)]
    fig = sequence_quality("planar 45x21", poses)
    assert fig["all"][1] < fig["all"][0]
    assert fig["followed"][1] < fig["followed"][0]


def test_quality_tiny0(scene_cache, sobol_matrices):
    """tiny0 100 x 75, the same four cameras as tests/test_temporal_definition.py: over all pixels the followed temporal result has the lower error.  The
    followed pixels alone are reported, not asserted: the mirror shows a strongly curved object.  Measured (DESIGN.md section 4 has the row): all px 0.2559 -> 0.2540,
    chain px 0.3816 -> 0.3912, followed px 0.3543 -> 0.3657 (worse: as measured), other px 0.2452 -> 0.2420; 84.3 % of the 427 followed pixels found history."""
    poses = [tiny0_pose(scene_cache, sobol_matrices, k, ref_spp=1024 if k == 3 else 0) for k in range(4)]
    fig = sequence_quality("tiny0 100x75", poses)
    assert fig["all"][1] < fig["all"][0]


def test_the_new_symbols_are_declared_and_bound():
    from adypt_amd import _native as N
    header = open(os.path.join(ROOT, "include", "adypt_hip.h")).read()
    for stem in ("denoise_temporal_specular", "read_denoise_virtual", "get_denoise_virtual"):
        for name in ("adypt_" + stem, "adypt_multi_" + stem):
            assert re.search(r"\bint %s\(" % name, header), name
            assert name in N.EXPORTS and hasattr(N.lib, name), name
    assert "typedef struct adypt_denoise_virtual" in header and C.sizeof(N.DenoiseVirtual) == 32


def test_the_chain_probes_edge_inputs_through_the_header(lib, tmp_path):
    """tests/chain_edge_inputs.py — what tests/test_gpu_chain_probes.py gives k_chain_start<true> and k_chain_step<true> — with the compiled header's
    chain_at_primary, chain_hit_point, chain_at_surface, chain_start_length, chain_unfold and chain_virtual_point in place of numpy's: the same states
    with their lengths, rays, guides and virtual points to the bit, and every case reaches what it is named after."""
    from tests import chain_edge_inputs as CE
    ops, lengths = SD.build_header(tmp_path), HeaderUnfold(lib)
    sc = CE.scene()
    for picture in CE.START_PICTURES:
        for n_blocks in (1, 2, 3):
            for pattern in CE.START_PATTERNS:
                case = CE.start_case(picture, n_blocks, pattern)
                want = CE.start_truth(sc, case, True)
                assert CE.start_reach(case, want), (picture, n_blocks, pattern)
                if want["go"].any():
                    assert (want["state"][want["go"], 1, 3] > 0).all(), "a followed pixel's camera ray has a length"
                SD.assert_same_arrays(CE.start_truth(sc, case, True, ops=ops, lengths=lengths), want, ("go", "hits_w", "state", "o", "d"), "start %s %d %s" % (picture, n_blocks, pattern))
    for name in CE.STEP_COUNTS:
        case = CE.step_case(name)
        want = CE.step_truth(sc, case, True)
        assert CE.step_reach(sc, case, want, True), name
        got = CE.step_truth(sc, case, True, ops=ops, lengths=lengths)
        SD.assert_same_arrays(got, want, ("albedo", "normal", "position", "hits", "state", "virt", "go"), "step " + name)
        SD.assert_same_arrays(dict(o=got["rays"][0], d=got["rays"][1]), dict(o=want["rays"][0], d=want["rays"][1]), ("o", "d"), "step %s: the rays" % name)
        assert (got["escaped"], got["truncated"]) == (want["escaped"], want["truncated"])
