"""The hand-made edge inputs of the kernels of a moments call and of the three later prepare instances, named once (not a test module):
k_denoise_prepare_class / _moments / _virtual, k_temporal_merge_moments<MOTION> and k_moments_variance.  Every entry carries `reach`, a function of its
inputs or of the TRUTH's outputs (never the code under test's) that says whether the branch the entry exists for is reached.
tests/test_moments_definition.py runs the entries through the headers on the CPU, tests/test_gpu_moments_probes.py through the kernels.  Built from
tests/denoise_edge_inputs.py and the generators of the definition tests, imported and not copied."""
import numpy as np

from tests import denoise_edge_inputs as E
from tests import denoise_truth as D
from tests import moments_truth as MT
from tests import temporal_motion_truth as TM
from tests.denoise_edge_inputs import rgba
from tests.probe import same as same_bits  # (equal bits, or NaN on both sides)
from tests.test_temporal_definition import camera_of, wall

F = np.float32
POISON = F(777.0)  # what the local pixels of an edge block outside the picture hold: it must reach no output
WG_X, WG_Y = 32, 8  # the workgroup of the image kernels
UNDER_2, UNDER_4 = np.nextafter(F(2), F(0)), np.nextafter(F(4), F(0))


# ---- the prepare instances ----
PREPARE_SIZES = [(1, 1), (33, 9), (70, 40)]
CLASS_WORDS = np.array([-9, -1, 0, 1, 2, 9, UNDER_2, np.nan, np.inf], np.float32)  # what hits.w may hold: the class word of the chain, or anything else


def prepare_case(w, h):
    """One picture for all three instances: C, m2, per-block n, A, N, P, the class word and the hit word of every pixel, and the virtual-point image."""
    rs = np.random.RandomState(201 + w)
    u = lambda lo, hi, *s: rs.uniform(lo, hi, size=s).astype(np.float32)  # noqa: E731
    nbx, nby = (w + 31) // 32, (h + 31) // 32
    C, m2, A, N, P, G = u(0, 2, h, w, 3), u(0.1, 3, h, w), u(0.1, 0.9, h, w, 3), u(-1, 1, h, w, 3), u(-3, 3, h, w, 3), u(-9, 9, h, w, 4)
    cls = CLASS_WORDS[(np.arange(h * w) % len(CLASS_WORDS)).reshape(h, w)].copy()
    word = E.hit_word_image(np.ones((h, w), bool))
    spp = np.array([1, 0, 1, 3, 2, 1], np.int32)[:nbx * nby]  # per block, ascending: n = 1, 0, 3, 2 side by side
    if w * h == 1:
        cls[0, 0], word[0, 0] = 2, -1  # the one pixel: followed by its class word, a miss by its hit word
        m2[:] = 0
    else:
        cls[2, 5], word[2, 5] = 1, -1  # .x says miss, .w says class 1: the class instances must not look at .x
        cls[3, 6], word[3, 6] = 0, 5   # and the reverse
        m2[:, 0:12] = 0                # n = 1 with m2 = 0 (block 0), and with m2 != 0 beside it
        A[1, 1:4], A[4, 2] = 0, F(-0.01)
        A[5, 3, 1] = F(-0.01)          # one channel's divisor 0, the luminance's not
        C[6, 4, 2], C[7, 7, 0] = np.nan, np.inf
    return dict(w=w, h=h, C=C, m2=m2, spp=spp, A=A, N=N, P=P, cls=cls, word=word, G=G)


def prepare_cases():
    return {"%dx%d" % s: prepare_case(*s) for s in PREPARE_SIZES}


def prepare_inputs(case, order):
    """the block-major arrays of the block list `order`; the local pixels outside the picture hold POISON everywhere"""
    w, h = case["w"], case["h"]
    bm = lambda img: E.block_major(img, order, w, h)  # noqa: E731
    pad = bm(np.ones((h, w, 4), np.float32))[:, 0] == 0
    hits = E.words_as_float4(case["word"])
    hits[..., 1:3] = 0.25
    hits[..., 3] = case["cls"]
    moments = rgba(np.stack([np.full((h, w), 0.5, np.float32), case["m2"], np.zeros((h, w), np.float32)], -1), 0.0)
    local = dict(accum=bm(rgba(case["C"], 1.0)), albedo=bm(rgba(case["A"], 1.0)), normal=bm(rgba(case["N"], 1.0)), position=bm(rgba(case["P"], 1.0)), hits=bm(hits),
                 virtual=bm(case["G"]), moments=bm(moments))
    for v in local.values():
        v[pad] = POISON
    local["moments"] = np.ascontiguousarray(local["moments"][:, :2])
    return dict(local, blocks=np.asarray(order, np.int32), block_spp=np.asarray(case["spp"], np.int32)[order], pad=pad)


def prepare_truth(case, instance):
    """X0, X1, X2, XA (and XV for the virtual instance) by denoise_truth.prepare / moments_truth.prepare and the rule of who has a virtual point"""
    w, h = case["w"], case["h"]
    n = D.block_counts(h, w, case["spp"])
    D0, W0, _ = (MT.prepare if instance == "moments" else D.prepare)(case["C"], case["m2"], n, case["A"])
    flag = (case["word"] != -1).astype(np.float32) if instance == "moments" else case["cls"]
    out = [rgba(D0, W0), rgba(case["N"], flag), rgba(case["P"], n), rgba(case["A"], 0.0)]
    if instance == "virtual":
        with np.errstate(invalid="ignore"):
            has = case["cls"] >= F(2)
        out.append(np.where(has[..., None], case["G"], rgba(case["P"], 0.0)).astype(np.float32))
    return out


def prepare_reach(case, instance):
    """from the inputs and the truth: the pixels the instance exists for are there, and another choice would give other words"""
    w, h, cls, word = case["w"], case["h"], case["cls"], case["word"]
    by_word = (word != -1).astype(np.float32)
    if w * h == 1:
        return bool(cls[0, 0] == 2 and by_word[0, 0] == 0 and case["spp"][0] == 1 and case["m2"][0, 0] == 0)
    t = prepare_truth(case, instance)
    if instance == "moments":
        n = D.block_counts(h, w, case["spp"])
        plain = D.prepare(case["C"], case["m2"], n, case["A"])[1]
        Y = D.lum(t[0][..., :3])
        at = (n == 1) & (case["m2"] == 0) & np.isfinite(Y)
        ok = at.any() and same_bits(Y[at] * Y[at], t[0][..., 3][at]).all()  # S0 is Y^2 to the bit
        ok = ok and ((n == 1) & (case["m2"] != 0)).any() and (w < 33 or (n == 0).any()) and (w < 70 or len(set(case["spp"].tolist())) == 4)
        ok = ok and not same_bits(t[0][..., 3], plain).all() and np.isnan(t[0][6, 4, 2]) and np.isfinite(t[0][1, 1]).all() and np.isinf(t[0][4, 2, :3]).all() and np.isinf(t[0][5, 3, 1])
        return bool(ok and (case["A"][4, 2] == F(-0.01)).all() and not same_bits(t[1][..., 3], cls).all())
    ok = all(same_bits(cls, np.full_like(cls, v)).any() for v in CLASS_WORDS) and cls[2, 5] == 1 and by_word[2, 5] == 0 and cls[3, 6] == 0 and by_word[3, 6] == 1
    if instance == "virtual":
        xv, own = t[4], rgba(case["P"], 0.0)
        with np.errstate(invalid="ignore"):
            gt, ge = cls > F(2), cls >= F(2)
        ok = ok and (same_bits(xv, own).all(-1) == ~ge).all() and (same_bits(xv, case["G"]).all(-1) == ge).all()  # XV is G exactly where class >= 2
        ok = ok and (ge & ~gt).any() and same_bits(xv[cls == UNDER_2], own[cls == UNDER_2]).all() and ge[np.isinf(cls)].all() and not ge[np.isnan(cls)].any()
    return bool(ok)


# ---- k_temporal_merge_moments: denoise_edge_inputs' temporal and motion cases with the fourth channel read as S, and what a moments call adds ----
def merge_cases():
    rs = np.random.RandomState(202)
    c = {}
    for name, case in E.temporal_cases().items():
        c["temporal/" + name] = case
    for name, case in E.motion_cases().items():
        c["motion/" + name] = case
    h, w = 9, 13
    cam = camera_of()
    full = E.history(wall(rs, h, w, cam), cam)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def add(name, call, hist, reach, **kw):
        c["moments/" + name] = dict(call=call, hist=hist, cam=cam, kw=kw, reach=reach)
        return c["moments/" + name]
    # a sub-pixel shift: four taps of unequal weight — a tap's S blended with w * w instead of w gives other words
    case = add("sub-pixel", wall(rs, h, w, cam, fx=xx + 0.37, fy=yy + 0.21), full, None)
    case["reach"] = lambda t, case=case: bool((t["n_out"][1:-2, 1:-2] > t["n"][1:-2, 1:-2]).all()
                                              and not same_bits(t["V"], merge_truth(case, square_tap_weight=True)["V"])[1:-2, 1:-2].any())

    # NaN and +-inf in the S, D and n of single history pixels: the tap is refused, nothing spreads
    def spoil(a, i):
        a[1 + i, 9], a[1 + i, 3], a[5 + i, 6] = np.nan, np.inf, -np.inf
    bad = E.altered(full, V=lambda a: spoil(a, 0), D=lambda a: spoil(a, 1), n=lambda a: spoil(a, 2))
    case = add("nan-inf-history", wall(rs, h, w, cam), bad, None)
    at = ([1, 2, 3, 1, 2, 3, 5, 6, 7], [9, 9, 9, 3, 3, 3, 6, 6, 6])
    case["reach"] = lambda t, case=case: bool(all(np.isfinite(t[k]).all() for k in ("n_out", "D", "V")) and (t["n_out"][at] == t["n"][at]).all()
                                              and (t["n_out"] > t["n"]).sum() == h * w - 9 and (merge_truth(case, full)["n_out"][at] > t["n"][at]).all())
    # have = 0 over a stale history in memory
    case = add("have-0", wall(rs, h, w, cam), None, None)
    case["stale"] = full
    case["reach"] = lambda t, case=case: bool((t["n_out"] == t["n"]).all() and same_bits(t["V"], E.images(case["call"])["V"]).all()
                                              and (merge_truth(case, full)["n_out"] > t["n"]).all())
    # a reprojection a hair outside each border, and a hair inside it
    # (0.011 and 0.009 inside a border: the one tap that counts weighs more and less than kTemporalMinWeight)
    ex = np.array([-1.001, -1.0, -0.991, -0.989, -0.5, 0.0, 5.25, w - 1.5, w - 1.0, w - 0.011, w - 0.009, w * 1.0, w + 0.001])
    ey = np.array([-1.001, -1.0, -0.989, 3.75, 4.5, h - 1.5, h - 0.011, h - 0.009, h * 1.0])
    fx, fy = np.broadcast_to(ex[None, :], (h, w)), np.broadcast_to(ey[:, None], (h, w))

    def border(t):
        took = t["n_out"] > t["n"]
        return bool(not took[:, :3].any() and not took[:, 10:].any() and not took[:2, :].any() and not took[7:, :].any() and took[3:6, 3:10].all() and took[2, 5:9].all()
                    and took[6, 5:9].all() and not took[2, 3] and not took[6, 9])
    add("border", wall(rs, h, w, cam, fx=fx, fy=fy), full, border)
    return c


def merge_through(case):
    """(N_prev, P_prev, valid) and the XP, XN images of a case: the motion cases' triangles say; every other case stands still"""
    im = E.images(case["call"])
    h, w = im["hit"].shape
    if "tri" in case:
        hist = case["hist"]
        Pp, moved, Np, valid = TM.previous_point(None if hist is None else hist.get("tris"), case["cur"], case["tri"], case["uv"], im["N"], im["P"])
    else:
        Pp, moved, Np, valid = im["P"], np.zeros((h, w), bool), im["N"], np.ones((h, w), bool)
    return (Np, Pp, valid), rgba(Pp, moved.astype(np.float32)), rgba(Np, valid.astype(np.float32)), moved


def merge_truth(case, hist="own", motion=False, **kw):
    """moments_truth.merge of a case (or of the case under another history), X0.w and the history's fourth channel read as S: dict(n, n_out, D, V)"""
    im = E.images(case["call"])
    through, _, _, moved = merge_through(case)
    if not motion and "tri" not in case:
        through = None
    Dm, Sm, no = MT.merge(im["D"], im["V"], im["n"], im["N"], im["P"], im["A"], im["hit"], case["hist"] if isinstance(hist, str) else hist, case["kw"].get("cap", 64.0), through=through, **kw)
    return dict(n=im["n"], n_out=no, D=Dm, V=Sm, moved=moved, valid=np.asarray(through[2]) if through is not None else np.ones_like(moved))


# ---- k_moments_variance ----
VARIANCE_SIZES = E.SIZES + [(33, 513)]


def variance_base(w, h, rs, n_out=1.0):
    """the merged images of a wall 5 in front of the camera: every pixel a hit on one plane with one albedo, S above lum(D)^2"""
    cam = camera_of(w=w, h=h)
    C, _, _, A, N, P, hit = wall(rs, h, w, cam)
    Y = D.lum(C)
    S = (Y * Y + rs.uniform(0.1, 1, size=(h, w)).astype(np.float32)).astype(np.float32)
    return dict(w=w, h=h, origin=cam[0], D=C, S=S, n_out=np.full((h, w), n_out, np.float32), N=N, P=P, A=A, hit=hit)


def variance_truth(case):
    """dict(V, spatial, k, asks, own) by moments_truth.variance"""
    V, spatial, k = MT.variance(case["D"], case["S"], case["n_out"], case["N"], case["P"], case["A"], case["hit"], case["origin"])
    with np.errstate(all="ignore"):
        asks = case["hit"] & (case["n_out"] < F(4))
        own = MT.variance(case["D"], case["S"], case["n_out"], case["N"], case["P"], case["A"], case["hit"], case["origin"], window=False)[0]
    return dict(V=V, spatial=spatial, k=k, asks=asks, own=own)


def variance_images(case):
    """merged, X1, X2, XA of the kernel"""
    return rgba(case["D"], case["S"]), rgba(case["N"], case["hit"].astype(np.float32)), rgba(case["P"], case["n_out"]), rgba(case["A"], 0.0)


def window_size(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((np.minimum(xx + 3, w - 1) - np.maximum(xx - 3, 0) + 1) * (np.minimum(yy + 3, h - 1) - np.maximum(yy - 3, 0) + 1)).astype(np.float32)


def workgroup_of(h, w):
    """(H, W) int: the workgroup index of every pixel"""
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy // WG_Y) * ((w + WG_X - 1) // WG_X) + xx // WG_X


def staged_workgroups(t, h, w):
    return np.unique(workgroup_of(h, w)[t["asks"]])


def variance_cases():
    rs = np.random.RandomState(203)
    c = {}

    def add(name, case, reach):
        c[name] = dict(case, reach=reach)
        return c[name]
    for w, h in VARIANCE_SIZES:
        # no pixel asks: nothing is staged, V = own / n
        add("none-asks-%dx%d" % (w, h), variance_base(w, h, rs, 8.0),
            lambda t: bool(not t["asks"].any() and not t["spatial"].any() and (t["V"] > 0).all()))
        # every pixel asks (1 x 1 and 3 x 2: the halo is outside on every side)
        add("all-ask-%dx%d" % (w, h), variance_base(w, h, rs, 1.0),
            lambda t, w=w, h=h: bool(t["asks"].all() and np.array_equal(t["k"], window_size(h, w)) and t["spatial"].all() == (w * h >= 4) and t["spatial"].any() == (w * h >= 4)))
    # 33 x 513 is 2 x 65 workgroups: the 64 count slots wrap twice; workgroup (bx, by) holds 1 + (by + bx) % 5 asking pixels, and every one of them decides
    w, h = 33, 513
    case = variance_base(w, h, rs, 8.0)
    yy, xx = np.mgrid[0:h, 0:w]
    want = 1 + (yy // WG_Y + xx // WG_X) % 5
    case["n_out"][np.where(xx < WG_X, (yy % WG_Y == 0) & (xx < want), yy % WG_Y < want)] = 1  # along the first row of a workgroup, down the one-pixel second column
    expected = np.zeros(130, np.int64)
    expected[workgroup_of(h, w)] = want
    add("slots-wrap-33x513", case, lambda t, expected=expected, w=w, h=h: bool(len(staged_workgroups(t, h, w)) == 130 and (expected >= 1).all() and np.array_equal(
        np.bincount(workgroup_of(h, w)[t["spatial"]], minlength=130), expected) and int(t["spatial"].sum()) == int(t["asks"].sum()) == int(expected.sum())))
    # exactly one asking pixel: every other workgroup is unstaged, and the window of the first two runs through three workgroups that do not stage
    for name, (w, h), (x, y) in (("one-asks-thread-0-0", (70, 40), (32, 8)), ("one-asks-thread-31-7", (70, 40), (63, 15)), ("one-asks-second-column-33x9", (33, 9), (32, 3)),
                                  ("one-asks-last-row-33x9", (33, 9), (5, 8))):
        case = variance_base(w, h, rs, 8.0)
        case["n_out"][y, x] = 2
        add(name, case, lambda t, x=x, y=y, w=w, h=h: bool(t["asks"].sum() == 1 and t["spatial"][y, x] and t["spatial"].sum() == 1 and t["k"][y, x] == window_size(h, w)[y, x]
                                                            and len(staged_workgroups(t, h, w)) == 1 and len(np.unique(workgroup_of(h, w)[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4])) == (4 if w == 70 else 2)
                                                            and not same_bits(t["V"][y, x], t["own"][y, x])))
    # an L of three hit pixels and a square of four, the rest sky, laid across the seams x = 31|32 and y = 7|8, 15|16: the window's taps come from the halo
    w, h = 70, 40
    case = variance_base(w, h, rs, 2.0)
    case["hit"][:] = False
    L3, SQ = [(7, 31), (7, 32), (8, 31)], [(15, 31), (15, 32), (16, 31), (16, 32)]
    for y, x in L3 + SQ:
        case["hit"][y, x] = True
    add("three-and-four-taps-across-seams", case, lambda t, w=w, h=h: bool(all(t["k"][p] == 3 and not t["spatial"][p] for p in L3) and all(t["k"][p] == 4 and t["spatial"][p] for p in SQ)
                                                                 and int(t["spatial"].sum()) == 4 and len(staged_workgroups(t, h, w)) == 6))
    # n_out on both sides of kMomentsMinLength, a NaN (does not ask), 0 on a hit (asks), and a miss centre with a short history (does not ask)
    w, h = 35, 11
    case = variance_base(w, h, rs, 8.0)
    lengths = np.array([4, UNDER_4, np.nan, 0, 1, 8, -1], np.float32)
    case["n_out"][:] = lengths[(np.arange(h * w) % len(lengths)).reshape(h, w)]
    case["hit"][case["n_out"] == 1] = False

    def by_length(t, n=case["n_out"]):
        with np.errstate(invalid="ignore"):
            return bool(not t["asks"][n == 4].any() and t["asks"][n == UNDER_4].all() and not t["asks"][np.isnan(n)].any() and t["asks"][n == 0].all() and not t["asks"][n == 1].any()
                        and t["spatial"][n == 0].all() and not np.isfinite(t["V"][n == 0]).any() and np.isnan(t["V"][np.isnan(n)]).all() and t["asks"][n == -1].all())
    add("lengths", case, by_length)
    # each refusal of moments_tap in turn: a spoilt region, and beside it a pixel whose window is short by exactly the region's taps
    reg, beside, inside = (slice(3, 6), slice(5, 8)), (4, 3), (4, 6)
    w, h = 13, 9
    normal = variance_base(w, h, rs)["N"][0, 0]
    turned = np.cross(normal, [0.3, 0.5, 0.8]).astype(np.float32)
    turned /= F(np.linalg.norm(turned))

    def f_hit(v): v["hit"][reg] = False
    def f_normal(v): v["N"][reg] = turned
    def f_plane(v): v["P"][reg] += normal * F(1.0)
    def f_albedo(v): v["A"][reg] += F(0.3)
    def f_inf_y(v): v["D"][reg] = np.inf
    def f_nan_s(v): v["S"][reg] = np.nan
    for name, spoil in (("refused-hit", f_hit), ("refused-normal", f_normal), ("refused-plane", f_plane), ("refused-albedo", f_albedo), ("refused-not-finite-Y", f_inf_y),
                        ("refused-not-finite-S", f_nan_s)):
        case = variance_base(w, h, rs, 1.0)
        spoil(case)
        add(name, case, lambda t, w=w, h=h: bool(t["k"][beside] == window_size(h, w)[beside] - F(6) and t["spatial"][beside]))
    # (a NaN S at the centre of its own window: the centre asks, is refused as its own tap, and takes the window of the eight others of the region's outside)
    c["refused-not-finite-S"]["reach"] = lambda t, w=w, h=h: bool(t["k"][beside] == window_size(h, w)[beside] - F(6) and t["asks"][inside] and t["k"][inside] == F(49 - 9) and t["spatial"][inside]
                                                         and np.isfinite(t["V"][inside]) and np.isfinite(t["V"][beside]))
    # S < lum(D)^2 (the floor): S = 0 under a long history, and under a short one whose window has too few taps to decide
    case = variance_base(w, h, rs, 10.0)
    case["S"][:] = 0
    case["n_out"][:, 5:], case["hit"][:, 5:] = 2, False
    case["hit"][2, 10] = True
    add("floor", case, lambda t: bool((t["V"] == 0).all() and not t["spatial"].any() and t["asks"][2, 10] and t["k"][2, 10] == 1 and not np.signbit(t["V"]).any()))
    return c
