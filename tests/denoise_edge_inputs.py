"""The denoiser's hand-made edge inputs, named once (not a test module).  Every entry says what a call sees (C, m2, n, A, N, P, hit — the inputs of the
numpy truths), what the history holds, the cameras and the parameters, and carries `reach`: a function of the TRUTH's outputs (never the code under
test's) that says whether the branch the entry exists for is reached.  The four tests/test_*_definition.py run the entries through the header on the CPU,
tests/test_gpu_denoise_probes.py runs them through the kernels.  Built from the generators of the definition tests, imported and not copied.

Hit flags are 0 or 1 throughout (the truths take them as bool); a history is what temporal_truth.commit makes, plus raw_cam (origin 3, inv_proj 16,
inv_view 16 floats) and, for a motion call's, tris."""
import numpy as np

from adypt_amd import distributed as DI
from tests import denoise_truth as D
from tests import rectify_truth as R
from tests import temporal_motion_truth as TM
from tests import temporal_truth as TT
from tests.test_denoise_definition import plane
from tests.test_rectify_definition import window_size
from tests.test_temporal_definition import camera_of, wall
from tests.test_temporal_motion_definition import scene as moved_scene

F = np.float32
BLOCK = 32
# (w, h) around the 32 x 8 workgroup and the halo of 3: 35 x 11 puts the halo of the second workgroup column and row wholly inside the image on one side
# and wholly outside on the other; 70 x 40 is 3 x 5 workgroups and 3 x 2 blocks, partial on both edges
SIZES = [(1, 1), (3, 2), (31, 7), (32, 8), (33, 9), (35, 11), (70, 40)]
SIGMAS = [(4.0, 0.1), (0.5, 2.0)]
STEPS = [1, 2, 4, 8, 16, 32]
MIN_TAPS = 4  # kRectifyMinTaps


# ---- a call's images ----
def counts(call):
    h, w = np.shape(call[1])
    return np.asarray(call[2], np.float32) if np.ndim(call[2]) == 2 else D.block_counts(h, w, call[2])


def images(call):
    """What prepare makes of a call, as the truths take it: D, V (X0), N, hit (X1), P, n (X2), A (XA)."""
    C, m2, _, A, N, P, hit = call
    n = counts(call)
    A, N, P = (np.ascontiguousarray(v, np.float32) for v in (A, N, P))
    D0, V0, ka = D.prepare(np.asarray(C, np.float32), m2, n, A)
    return dict(D=D0, V=V0, n=n, N=N, P=P, A=A, hit=np.asarray(hit).astype(bool), ka=ka)


def rgba(rgb, w):
    """(H, W, 4) float32 from (H, W, 3) and the fourth channel (an (H, W) array or a number)"""
    h, wd = rgb.shape[:2]
    return np.ascontiguousarray(np.concatenate([np.asarray(rgb, np.float32), np.broadcast_to(np.asarray(w, np.float32), (h, wd))[..., None]], -1))


def x_images(im):
    """X0, X1, X2, XA of the kernels"""
    return rgba(im["D"], im["V"]), rgba(im["N"], im["hit"].astype(np.float32)), rgba(im["P"], im["n"]), rgba(im["A"], 0.0)


def h_images(hist, h, w):
    """H0, H1, H2, HA and the raw camera of a history (zeros for none)"""
    if hist is None:
        z = np.zeros((h, w, 4), np.float32)
        return (z, z, z, z), (np.zeros(3, np.float32), np.zeros(16, np.float32), np.zeros(16, np.float32))
    raw = np.asarray(hist["raw_cam"], np.float32)
    return x_images(hist), (raw[0:3], raw[3:19], raw[19:35])


def history(call, cam, hist=None, tris=None, **kw):
    """the history a committing call leaves (temporal_truth's own), with the camera's raw numbers beside it"""
    _, _, new = TT.denoise(*call, hist, cam, levels=1, **kw)
    new["raw_cam"] = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in cam])
    if tris is not None:
        new["tris"] = np.array(tris, np.float32).reshape(-1, TM.TRI_WORDS)
    return new


def altered(hist, **fields):
    """a copy of a history with f(array) applied to the fields named"""
    new = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in hist.items()}
    for k, f in fields.items():
        f(new[k])
    return new


def rough(call, rs, misses=True):
    """a plane's call with tilted normals, an uneven surface and a sprinkle of misses: every edge-stopping weight of a level says something"""
    _, _, _, A, N, P, hit = call
    h, w = hit.shape
    N += rs.normal(0, 0.15, N.shape).astype(np.float32)
    N /= np.sqrt((N * N).sum(-1, keepdims=True)).astype(np.float32)
    P[..., 2] += rs.uniform(0, 0.05, (h, w)).astype(np.float32)
    if misses and h * w >= 6:
        m = rs.uniform(size=(h, w)) < 0.12
        m[0, 0] = False
        hit[m] = False
        A[m], N[m], P[m] = 0, 0, 0
    return call


# ---- prepare and the levels (denoise.hpp) ----
def filter_cases():
    rs = np.random.RandomState(101)
    c = {}

    def add(name, call, reach=lambda: True):
        c[name] = dict(call=call, reach=reach)
    for w, h in SIZES:
        add("rough-%dx%d" % (w, h), rough(plane(h, w, rs), rs))
    add("plane-2x3", plane(2, 3, rs))
    add("sky", plane(9, 13, rs, hit=False))
    call = plane(9, 13, rs, var=False)
    add("zero-variance", call, lambda m2=call[1]: bool((m2 == 0).all()))
    call = plane(10, 12, rs)
    call[3][2:6, 3:9] = 0
    call[6][4, 4] = False
    add("albedo-0", call, lambda A=call[3], hit=call[6]: bool(((A == 0).all(-1) & hit).any()))
    call = plane(11, 11, rs)
    call[6][4:7, 4:7] = False
    call[6][5, 5] = True
    call[6][9, 2] = False
    add("hit-among-misses", call)
    call = plane(12, 12, rs)
    call[4][6, 6] = np.nan
    call[4][0, 0, 1] = np.nan
    call[5][3, 8, 2] = np.nan
    add("nan-normal-position", call)
    call = rough(plane(40, 70, rs), rs)
    call[2] = np.array([2, 64, 3, 17, 5, 64], np.int32)  # n = 2 in one block and 64 in its neighbour
    add("counts-2-64", call, lambda n=call[2]: n[0] == 2 and n[1] == 64)
    call = plane(11, 35, rs)
    call[0][2, 3, 0], call[0][5, 33, 1], call[0][9, 0, 2], call[1][4, 4] = np.inf, np.nan, -np.inf, np.inf
    add("accum-inf-nan", call, lambda C=call[0]: bool(np.isinf(C).any() and np.isnan(C).any()))
    return c


def block_orders(w, h):
    """the block lists a picture is prepared with: ascending, reversed, and rank-major for 3 shards (the several-device path's upload order)"""
    nbx, nby = (w + BLOCK - 1) // BLOCK, (h + BLOCK - 1) // BLOCK
    asc = np.arange(nbx * nby, dtype=np.int32)
    rank3 = np.array([b for r in range(3) for b in asc if (b % nbx + b // nbx) % 3 == r], np.int32)
    return {"ascending": asc, "reversed": asc[::-1].copy(), "rank-major-3": rank3}


def block_major(img, order, w, h):
    """(H, W, 4) -> the block-major array of the block list `order` (distributed.tile_from_image's layout)"""
    t = DI.tile_from_image(np.ascontiguousarray(img, np.float32), 0, 1).reshape(-1, BLOCK * BLOCK, 4)
    return np.ascontiguousarray(t[order].reshape(-1, 4))


HIT_WORDS = np.array([0, 5, -2, -7, 2 ** 31 - 1, 3], np.int32)  # what a hit pixel's word may be: anything but -1, a known triangle or not


def hit_word_image(hit):
    h, w = hit.shape
    words = HIT_WORDS[(np.arange(h * w) % len(HIT_WORDS)).reshape(h, w)]
    return np.where(hit, words, np.int32(-1)).astype(np.int32)


def words_as_float4(words):
    """(H, W) int32 -> the primary-hit float4 image whose .x holds the word as bits (u, v, t in the rest: zeros here)"""
    out = np.zeros(words.shape + (4,), np.float32)
    out[..., 0] = words.astype(np.int32).view(np.float32)
    return out


def prepare_inputs(call, order, rs):
    """the block-major arrays k_denoise_prepare reads for a call whose n is a number or one count per block"""
    C, m2, n, A, N, P, hit = call
    h, w = hit.shape
    per_block = np.full(len(order), n, np.int32) if np.ndim(n) == 0 else np.asarray(n, np.int32)[order]
    moments = rgba(np.stack([rs.uniform(0, 1, (h, w)).astype(np.float32), np.asarray(m2, np.float32), np.zeros((h, w), np.float32)], -1), 0.0)
    local = {k: block_major(rgba(v, 1.0), order, w, h) for k, v in (("accum", C), ("albedo", A), ("normal", N), ("position", P))}
    local["moments"] = np.ascontiguousarray(block_major(moments, order, w, h)[:, :2])
    local["hits"] = block_major(words_as_float4(hit_word_image(np.asarray(hit).astype(bool))), order, w, h)
    return dict(local, blocks=order, block_spp=per_block)


# ---- the temporal merge (temporal.hpp) ----
def merge_truth(case, hist="own"):
    """temporal_truth.merge of a case (or of the case under another history): dict(n, n_out, D, V)"""
    im = images(case["call"])
    Dm, Vm, no = TT.merge(im["D"], im["V"], im["n"], im["N"], im["P"], im["A"], im["hit"], case["hist"] if isinstance(hist, str) else hist, case["kw"].get("cap", 64.0))
    return dict(n=im["n"], n_out=no, D=Dm, V=Vm)


def temporal_cases():
    rs = np.random.RandomState(102)
    c = {}

    def add(name, call, hist, cam, reach, **kw):
        c[name] = dict(call=call, hist=hist, cam=cam, kw=kw, reach=reach)
        return c[name]
    h, w = 9, 13
    cam = camera_of()
    full = history(wall(rs, h, w, cam), cam)
    # no history — but "stale": what lies in the history's memory all the same, as after adypt_denoise_history_reset; taken for a history it would be merged
    case = add("have-0", wall(rs, h, w, cam), None, cam, None)
    case["stale"] = full
    case["reach"] = lambda t, case=case: bool((t["n_out"] == t["n"]).all() and (merge_truth(case, full)["n_out"] > t["n"]).all())
    for sw_, sh in SIZES:
        scam = camera_of(w=sw_, h=sh)
        add("size-%dx%d" % (sw_, sh), wall(rs, sh, sw_, scam), history(wall(rs, sh, sw_, scam), scam), scam, lambda t: bool((t["n_out"] > t["n"]).mean() > 0.5))
    sky = wall(rs, h, w, cam)
    sky[6][:] = False
    for k in (3, 4, 5):
        sky[k][:] = 0
    add("sky", sky, history(sky, cam), cam, lambda t: bool((t["n_out"] == t["n"]).all()))
    call = wall(rs, h, w, cam)
    call[6][2:5, 3:8] = False
    add("call-miss", call, full, cam, lambda t, hit=call[6]: bool((t["n_out"][~hit] == t["n"][~hit]).all() and (t["n_out"][hit] > t["n"][hit]).any()))
    add("cap-below-n", wall(rs, h, w, cam), full, cam, lambda t: bool((t["n_out"] == t["n"] + F(2)).all()), cap=2.0)
    back = camera_of(yaw=200.0)
    add("turned-180", wall(rs, h, w, cam), history(wall(rs, h, w, back), back), cam, lambda t: bool((t["n_out"] == t["n"]).all()))
    # the reprojection on the image border and just outside it, on all four sides
    edge_x = np.array([-1.5, -1.001, -1.0, -0.999, -0.5, 0.0, 5.25, w - 1.5, w - 1.001, w - 1.0, w - 0.999, w - 0.5, w + 0.5])
    edge_y = np.array([-1.5, -1.0, -0.999, -0.5, 3.75, h - 1.001, h - 1.0, h - 0.5, h + 0.5])
    fx, fy = np.broadcast_to(edge_x[None, :], (h, w)), np.broadcast_to(edge_y[:, None], (h, w))

    def border(t):
        took = t["n_out"] > t["n"]
        return bool(not took[:, 0].any() and not took[:, -1].any() and not took[0, :].any() and not took[-1, :].any() and took[3:8, 4:12].all())
    add("border", wall(rs, h, w, cam, fx=fx, fy=fy), full, cam, border)
    # NaN in the call's P and N, NaN or Inf in every field of the history
    call = wall(rs, h, w, cam)
    call[5][2, 3, 1] = np.nan
    call[4][6, 7, 0] = np.nan

    def spoil(field, i):
        def f(a):
            a[1 + i, 9] = np.nan
            a[1 + i, 3] = np.inf
        return f
    bad = altered(full, **{k: spoil(k, i) for i, k in enumerate(("D", "V", "n", "P", "N", "A"))})
    case = add("nan-history", call, bad, cam, None)
    case["reach"] = lambda t, case=case: bool(np.isfinite(t["n_out"]).all() and t["n_out"][2, 3] == t["n"][2, 3] and (t["n_out"] != merge_truth(case, full)["n_out"]).any())
    # an emitter's history tap (albedo 0, demodulated by the floor) beside a lit wall, seen half a pixel to the side
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    before = wall(rs, h, w, cam)
    before[3][:, 6] = 0
    before[0][:, 6] = 50.0
    before[2] = np.full((h, w), 8, np.float32)
    before[2][:, 6] = 100
    add("emitter-tap", wall(rs, h, w, cam, fx=xx + 0.5), history(before, cam), cam, lambda t: bool((t["n_out"][:, 5] < F(16.1)).all() and (t["n_out"][:, 5] > F(15.9)).all()))
    # the plane moved along its normal by less and by more than the tolerance (0.02 of the distance 5)
    add("plane-moved-0.05", wall(rs, h, w, cam, depth=4.95), full, cam, lambda t: bool((t["n_out"][2:-2, 2:-2] > t["n"][2:-2, 2:-2]).all()))
    add("plane-moved-0.2", wall(rs, h, w, cam, depth=4.8), full, cam, lambda t: bool((t["n_out"] == t["n"]).all()))
    # every refusal of a tap in turn: the history is spoilt in a region; inside it (all four taps spoilt) no history is taken, where the whole history gives one
    reg, inner = (slice(2, 5), slice(3, 8)), (slice(3, 4), slice(4, 7))
    normal = full["N"][0, 0]

    def f_hit(a): a[reg] = False
    def f_normal(a): a[reg] = np.cross(normal, [0.3, 0.5, 0.8]).astype(np.float32) / F(np.linalg.norm(np.cross(normal, [0.3, 0.5, 0.8])))
    def f_plane(a): a[reg] += normal * F(1.0)
    def f_albedo(a): a[reg][..., 1] += F(0.2)
    def f_inf(a): a[reg] = np.inf
    def f_zero(a): a[reg] = 0
    def f_neg(a): a[reg] = -3.0
    for name, fields in (("tap-miss", dict(hit=f_hit)), ("tap-normal", dict(N=f_normal)), ("tap-plane", dict(P=f_plane)), ("tap-albedo", dict(A=f_albedo)),
                         ("tap-not-finite-D", dict(D=f_inf)), ("tap-not-finite-V", dict(V=f_inf)), ("tap-n-0", dict(n=f_zero)), ("tap-n-negative", dict(n=f_neg)),
                         ("tap-n-inf", dict(n=f_inf))):
        case = add(name, wall(rs, h, w, cam), altered(full, **fields), cam, None)
        case["reach"] = lambda t, case=case: bool((t["n_out"][inner] == t["n"][inner]).all() and (merge_truth(case, full)["n_out"][inner] > t["n"][inner]).all())
    # sw just below and just above kTemporalMinWeight: the pixel aims 0.9905 / 0.9895 of a pixel to the right of a history pixel that counts, and the other
    # three taps are misses (the history hits on even columns of even rows only): sw is 0.0095 / 0.0105
    board = np.zeros((h, w), bool)
    board[0::2, 0::2] = True
    sparse = altered(full, hit=lambda a: a.__setitem__(slice(None), board))
    at = (slice(2, h, 2), slice(0, w - 1, 2))  # (row 0 aims a hair above or below the border: left out)
    for name, off, takes in (("min-weight-below", 0.9905, False), ("min-weight-above", 0.9895, True)):
        case = add(name, wall(rs, h, w, cam, fx=xx + off), sparse, cam, None)
        case["reach"] = lambda t, case=case, takes=takes: bool(((t["n_out"][at] > t["n"][at]) == takes).all() and (merge_truth(case, full)["n_out"][at] > t["n"][at]).all())
    return c


# ---- the window statistics and the rectified merge (rectify.hpp) ----
def rectify_truth(case, call=None):
    """the window statistics and the rectified merge of a case (or of another call under the case's history and parameters)"""
    im = images(case["call"] if call is None else call)
    kw = case["kw"]
    R0, R1 = R.window(im["D"], im["V"], im["N"], im["P"], im["A"], im["hit"], case["cam"][0], kw.get("radius", 3))
    Dm, Vm, no, kept = R.merge(im["D"], im["V"], im["n"], im["N"], im["P"], im["A"], im["hit"], case["hist"], R0, R1, kw.get("gamma", 1.0), kw.get("cap", 64.0))
    return dict(n=im["n"], n_out=no, D=Dm, V=Vm, kept=kept, R0=R0, R1=R1)


def rectify_cases():
    rs = np.random.RandomState(103)
    c = {}

    def add(name, call, hist, cam, reach, **kw):
        c[name] = dict(call=call, hist=hist, cam=cam, kw=kw, reach=reach)
        return c[name]
    for sw_, sh in SIZES:
        scam = camera_of(w=sw_, h=sh)
        few = sw_ * sh < MIN_TAPS
        add("size-%dx%d" % (sw_, sh), wall(rs, sh, sw_, scam), history(wall(rs, sh, sw_, scam), scam), scam,
            lambda t, sw_=sw_, sh=sh, few=few: bool(np.array_equal(t["R0"][..., 3], window_size(sh, sw_, 3)) and (t["R0"][..., 3] < F(MIN_TAPS)).all() == few))
    h, w = 9, 13
    cam = camera_of()
    full = history(wall(rs, h, w, cam), cam)
    case = add("have-0", wall(rs, h, w, cam), None, cam, None)
    case["stale"] = full  # (what lies in the history's memory all the same)
    case["reach"] = lambda t, case=case: bool((t["n_out"] == t["n"]).all() and (t["kept"] == 1).all() and (rectify_truth(dict(case, hist=full))["n_out"] > t["n"]).any())
    # a hit centre whose window holds fewer than kRectifyMinTaps counting taps: a hit among misses
    call = wall(rs, h, w, cam)
    call[6][1:8, 3:10] = False
    call[6][4, 6] = True
    add("hit-among-misses", call, full, cam, lambda t: bool(t["R0"][4, 6, 3] == F(1) and t["kept"][4, 6] == F(1) and t["n_out"][4, 6] > t["n"][4, 6]))
    # taps refused by each of the five tests of rectify_tap in turn: a spoilt region, and beside it a pixel whose window is short by exactly the region's taps
    reg = (slice(3, 6), slice(5, 8))
    beside = (4, 3)  # its radius-3 window holds columns 0..6 of rows 1..7: 3 x 2 pixels of the region
    normal = full["N"][0, 0]
    turned = np.cross(normal, [0.3, 0.5, 0.8]).astype(np.float32)
    turned /= F(np.linalg.norm(turned))

    def f_miss(call): call[6][reg] = False
    def f_normal(call): call[4][reg] = turned
    def f_plane(call): call[5][reg] += normal * F(1.0)
    def f_albedo(call): call[3][reg] += F(0.3)
    def f_inf(call): call[0][reg] = np.inf
    def f_nan_v(call): call[1][reg] = np.nan
    for name, spoil in (("refused-miss", f_miss), ("refused-normal", f_normal), ("refused-plane", f_plane), ("refused-albedo", f_albedo), ("refused-not-finite-D", f_inf),
                        ("refused-not-finite-V", f_nan_v)):
        call = wall(rs, h, w, cam)
        spoil(call)
        add(name, call, full, cam, lambda t: bool(t["R0"][beside + (3,)] == window_size(h, w, 3)[beside] - F(6)))
    # window sums that overflow: radiance 2.9e38 in two taps — the mean is inf, the variance inf - inf is floored to 0, the history of every pixel that sees
    # both taps lies infinitely far from the mean and is dropped
    call = wall(rs, h, w, cam)
    call[0][4, 5:7] = F(1.5e38)

    def overflow(t):
        over = np.isinf(t["R0"][..., 0])
        return bool(over.sum() >= 20 and (t["kept"][over] == 0).all() and (t["n_out"][over] == t["n"][over]).all() and (t["kept"][~over] > 0).any())
    add("overflow", call, full, cam, overflow)
    # a limit that is a NaN: a tap whose square overflows makes g infinite, and gamma 0 times infinity is no number — the history is dropped
    call = wall(rs, h, w, cam)
    call[0][4, 6] = F(1.0e20)

    def limit_nan(t):
        over = np.isinf(t["R1"][..., 0])
        return bool(over.sum() >= 20 and (t["kept"][over] == 0).all() and (t["n_out"][over] == t["n"][over]).all())
    add("limit-nan", call, full, cam, limit_nan, gamma=0.0)
    # a history clamped in one channel only: the window's mean plus 3 limits in red, plus a tenth of a limit in green and blue
    call = wall(rs, h, w, cam)
    case = add("clamped-one-channel", call, None, cam, None)
    t0 = rectify_truth(dict(case, hist=None))
    lim = np.sqrt(t0["R1"][..., :3])
    case["hist"] = altered(full, D=lambda a: a.__setitem__(slice(None), (t0["R0"][..., :3] + lim * F([3.0, 0.1, 0.1])).astype(np.float32)))

    def one_channel(t, case=case):
        d = np.abs(case["hist"]["D"] - t["R0"][..., :3])
        l = np.sqrt(t["R1"][..., :3])
        return bool((d[..., 0] > l[..., 0]).all() and (d[..., 1:] <= l[..., 1:]).all() and ((t["kept"] > 0) & (t["kept"] < 1)).all())
    case["reach"] = one_channel
    add("gamma-0", wall(rs, h, w, cam), full, cam, lambda t: bool((t["kept"] == 0).all() and (t["n_out"] == t["n"]).all()), gamma=0.0)
    add("gamma-1e6-radius-1-cap-3", wall(rs, h, w, cam), full, cam, lambda t: bool((t["kept"] == 1).all() and (t["n_out"] == t["n"] + F(3)).all()), gamma=1.0e6, radius=1, cap=3.0)
    # kept reaching 0: a flat wall (limit 0) and a history that differs — the pixel takes no history
    floor = F(0.5) + F(0.01)
    flat, other = wall(rs, h, w, cam), wall(rs, h, w, cam)
    flat[0][:], flat[1][:], other[0][:], other[1][:] = floor * F(2.0), 0, floor * F(0.5), 0
    add("kept-0", flat, history(other, cam), cam, lambda t: bool((t["R1"] == 0).all() and (t["kept"] == 0).all() and (t["n_out"] == t["n"]).all()))
    add("kept-1-flat", flat, history(flat, cam), cam, lambda t: bool((t["kept"] == 1).all() and (t["n_out"] == F(16)).all()))
    # an emitter column next to a wall: the albedo test keeps it out of the wall's statistics
    scene = wall(rs, h, w, cam)
    scene[3][:, 6] = 0
    scene[0][:, 6] = 50.0
    add("emitter-column", scene, history(scene, cam), cam, lambda t: bool(np.array_equal(t["R0"][:, 6, 3], window_size(h, 1, 3)[:, 0]) and t["R0"][:, 6, :3].min() > 4000.0))
    return c


# ---- following moved geometry: the merge through XP, XN ----
def motion_truth(case):
    im = images(case["call"])
    prev = None if case["hist"] is None else case["hist"].get("tris")
    Pp, moved, Np, valid = TM.previous_point(prev, case["cur"], case["tri"], case["uv"], im["N"], im["P"])
    Dm, Vm, no = TT.merge(im["D"], im["V"], im["n"], Np, Pp, im["A"], im["hit"] & valid, case["hist"], case["kw"].get("cap", 64.0))
    return dict(n=im["n"], n_out=no, D=Dm, V=Vm, Pp=Pp, Np=Np, moved=moved, valid=valid)


def motion_cases():
    before, cam, after, tri, uv, prev, cur, region = moved_scene()
    hist = history(before, cam, tris=prev)
    c = {}
    for name, call, hs, now, reach in (
            ("first-call", before, None, prev, lambda t: bool(not t["moved"].any() and (t["n_out"] == t["n"]).all())),
            # moved triangles find their history; a zero-length previous normal gives XN.w = 0: no history
            ("moved", after, hist, cur, lambda t: bool(t["moved"].any() and (~t["valid"]).any() and (t["n_out"][~t["valid"]] == t["n"][~t["valid"]]).all()
                                                       and (t["n_out"][t["moved"]] > t["n"][t["moved"]]).any())),
            ("records-unchanged", after, hist, prev, lambda t: bool(not t["moved"].any())),
            ("no-snapshot", after, {k: v for k, v in hist.items() if k != "tris"}, cur, lambda t: bool(not t["moved"].any()))):
        c[name] = dict(call=call, hist=hs, cam=cam, tri=tri, uv=uv, cur=now, kw={}, reach=reach)
    c["moved-cap-3"] = dict(c["moved"], kw=dict(cap=3.0))
    c["first-call"]["stale"] = hist  # (what lies in the history's memory all the same: the call's own pose, which it would merge with)
    assert (motion_truth(dict(c["first-call"], hist=hist))["n_out"] > F(8)).any()
    return c


# ---- k_motion_gather ----
GATHER_KNOWN = 6
SLACK_VALUE = F(12345.0)  # what the probe fills the slack round the gather's tables with
POISON = F(777.0)         # what words 20..31 of a record hold: it must reach neither a snapshot nor a previous point


def gather_tables(rs, n_known=GATHER_KNOWN, extra=8):
    """(snapshot (n_known, 20), records (n_known + extra, 32)): triangle 0 unmoved (18 equal words), 1 differs in the last bit of word 17 only, 2 moved,
    3 with previous normals that sum to 0, 4 with previous normals holding Inf, 5 (= n_known - 1) moved; the records beyond are strangers."""
    records = np.full((n_known + extra, 32), POISON, np.float32)
    records[:, :20] = rs.uniform(-2, 2, (n_known + extra, 20)).astype(np.float32)
    snapshot = records[:n_known, :20].copy()
    if n_known >= GATHER_KNOWN:
        snapshot[1, 17] = (snapshot[1:2, 17].view(np.uint32) ^ np.uint32(1)).view(np.float32)[0]
        snapshot[2, :18] += F(0.25)
        snapshot[3, :9] += F(0.5)
        snapshot[3, 9:18] = 0
        snapshot[4, :9] -= F(0.5)
        snapshot[4, 12] = np.inf
        snapshot[5, :18] = rs.uniform(-2, 2, 18).astype(np.float32)
    return snapshot, records


def gather_words(n_known):
    """the hit words the gather is given: sky, the first and the last known triangle, the first stranger, strangers on both sides (never farther than 32
    from either end of [0, n_known))"""
    return np.unique(np.array([-1, 0, max(n_known - 1, 0), n_known, n_known + 5, -2, -7] + list(range(min(n_known, GATHER_KNOWN))), np.int32))


def gather_cases():
    rs = np.random.RandomState(104)
    c = {}
    for name, (w, h), n_known in (("35x11", (35, 11), GATHER_KNOWN), ("70x40", (70, 40), GATHER_KNOWN), ("3x2", (3, 2), GATHER_KNOWN), ("n_known-0", (35, 11), 0)):
        snapshot, records = gather_tables(rs, n_known)
        words = gather_words(n_known)
        tri = words[rs.randint(0, len(words), (h, w))]
        tri.reshape(-1)[:len(words)] = words[:h * w]  # every word at least once where the picture has room
        uv = rs.uniform(0, 0.5, (h, w, 2)).astype(np.float32)
        corners = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0.5]], np.float32)  # u, v at 0, 1 and (0.5, 0.5) on four pixels in six
        pick = rs.randint(0, 6, (h, w))
        for k in range(4):
            uv[pick == k] = corners[k]
        N = rs.normal(0, 1, (h, w, 3)).astype(np.float32)
        P = rs.uniform(-3, 3, (h, w, 3)).astype(np.float32)
        c[name] = dict(w=w, h=h, tri=tri.astype(np.int32), uv=uv, N=N, P=P, snapshot=snapshot, records=records, n_known=n_known)
    return c


def gather_truth(case):
    prev = case["snapshot"][:, :TM.TRI_WORDS] if case["n_known"] else None
    Pp, moved, Np, valid = TM.previous_point(prev, case["records"][:, :TM.TRI_WORDS], case["tri"], case["uv"], case["N"], case["P"])
    return rgba(Pp, moved.astype(np.float32)), rgba(Np, valid.astype(np.float32)), moved, valid


def gather_inputs(case, order):
    w, h = case["w"], case["h"]
    hits = words_as_float4(case["tri"])
    hits[..., 1:3] = case["uv"]
    hits = block_major(hits, order, w, h)
    pad = block_major(np.ones((h, w, 4), np.float32), order, w, h)[:, 0] == 0  # local pixels outside the picture: sky
    hits[pad, 0] = np.array([-1], np.int32).view(np.float32)[0]
    return dict(hits=hits, normal=block_major(rgba(case["N"], 0.0), order, w, h), position=block_major(rgba(case["P"], 0.0), order, w, h))


# ---- k_motion_snapshot ----
SNAPSHOT_COUNTS = [1, 63, 64, 65, 129]


def snapshot_records(n):
    """n records of 32 words: words 0..19 are what a snapshot keeps, words 20..31 hold POISON"""
    rs = np.random.RandomState(105 + n)
    records = np.full((n, 32), POISON, np.float32)
    records[:, :20] = rs.uniform(-2, 2, (n, 20)).astype(np.float32)
    records[0, 3], records[n - 1, 19] = np.nan, np.inf
    return records
