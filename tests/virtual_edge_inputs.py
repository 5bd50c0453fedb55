"""The hand-made edge inputs of the merge by the virtual point, named once (not a test module): raw images as k_temporal_merge_virtual takes them — X0 =
(D, V), X1 = (N, class), X2 = (P, n), XA = (A, .), XV = (Pv, len), the history H0 H1 H2 HA with classes in H1.w — and `reach`, a function of the TRUTH's
n_out that says whether the entry reaches what it is named after.  tests/test_virtual_definition.py runs them through the header on the CPU,
tests/test_gpu_virtual_probe.py through the kernel.

The picture: the history's camera saw a wall 5 in front of it, every pixel of class 2; the current call's followed point lies on that wall too (so the
plane, normal and albedo tests pass wherever they are asked) while its virtual point lies 9 in front of the history's camera at the pixel coordinates
(fx, fy) the entry aims at: where the history is fetched is decided by Pv alone."""
import numpy as np

from tests import temporal_truth as TT
from tests import virtual_truth as V
from tests.denoise_edge_inputs import rgba
from tests.test_temporal_definition import camera_of, cast

F = np.float32
SIZE = (33, 9)  # one column and one row more than the 32 x 8 workgroup
N_CALL, N_HIST = 4.0, 8.0


def base(w, h, fx=None, fy=None, seed=3):
    rs = np.random.RandomState(seed)
    cam = camera_of(w=w, h=h)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    fx, fy = xx if fx is None else fx, yy if fy is None else fy
    Pq, Nq = cast(cam, w, h, xx, yy, 5.0)
    P, N = cast(cam, w, h, fx, fy, 5.0)
    Pv, _ = cast(cam, w, h, fx, fy, 9.0)
    length = np.sqrt(((Pv.astype(np.float64) - cam[0].astype(np.float64)) ** 2).sum(-1)).astype(np.float32)
    u = lambda lo, hi, *s: rs.uniform(lo, hi, size=s).astype(np.float32)  # noqa: E731
    two = np.full((h, w), 2.0, np.float32)
    case = dict(w=w, h=h, cam=cam, cap=64.0, have=1,
                x0=rgba(u(0, 2, h, w, 3), u(0, 1, h, w)), x1=rgba(N, two), x2=rgba(P, N_CALL), xa=rgba(np.full((h, w, 3), 0.5, np.float32), 0.0), xv=rgba(Pv, length),
                h0=rgba(u(0, 2, h, w, 3), u(0, 1, h, w)), h1=rgba(Nq, two), h2=rgba(Pq, N_HIST), ha=rgba(np.full((h, w, 3), 0.5, np.float32), 0.0))
    return case


def cases(size=SIZE):
    w, h = size
    out = {}
    # every pixel aims at its own place: all take history
    c = base(w, h)
    c["reach"] = lambda n: (n > F(N_CALL)).all()
    out["own_place"] = c
    # one tap off each image edge, and wholly outside
    ex = np.array([-1.5, -1.001, -1.0, -0.999, -0.5, 0.0, 5.25] + [10.5] * (w - 13) + [w - 1.5, w - 1.001, w - 1.0, w - 0.999, w - 0.5, w + 0.5])
    ey = np.array([-1.5, -1.0, -0.999, -0.5, 3.75, h - 1.001, h - 1.0, h - 0.5, h + 0.5][:h])
    assert len(ex) == w and len(ey) == h
    c = base(w, h, np.broadcast_to(ex[None, :], (h, w)), np.broadcast_to(ey[:, None], (h, w)))
    # (a pixel aimed 0.999 outside brings a weight of 0.001, below the least weight: columns 0..3, rows 0..2 and the last of each take nothing)
    c["reach"] = lambda n: not (n[:, :4] > F(N_CALL)).any() and not (n[:, -1] > F(N_CALL)).any() and not (n[:3] > F(N_CALL)).any() and not (n[-1] > F(N_CALL)).any() and (n[3:8, 4:w - 1] > F(N_CALL)).all()
    out["off_each_edge"] = c
    # classes: a tap of another class is refused; a class 1 pixel goes through its own P; classes <= 0 and a NaN class take nothing
    c = base(w, h)
    c["h1"][:, 4, 3] = 3.0                       # the history holds another class in column 4 ...
    c["x1"][:, 8, 3], c["h1"][:, 8, 3] = 3.0, 3.0  # ... and the same other class in column 8
    c["x1"][:, 12, 3], c["h1"][:, 12, 3] = 1.0, 1.0
    c["xv"][:, 12] = c["x2"][:, 12] * np.array([1, 1, 1, 0], np.float32)  # (P, 0), as prepare leaves a pixel that is not followed
    c["x1"][:, 14, 3] = 1.0                      # class 1 now, class 2 then
    c["x1"][:, 16, 3] = 0.0
    c["x1"][:, 18, 3] = -2.0
    c["x1"][:, 20, 3] = np.nan
    c["reach"] = lambda n: (not (n[:, [4, 14, 16, 18, 20]] > F(N_CALL)).any()) and (n[:, [8, 12]] > F(N_CALL)).all() and (n[:, 2] > F(N_CALL)).all()
    out["classes"] = c
    # the virtual point's length: 0 (not valid), an infinity (the unfolded length overflowed), a NaN, negative
    c = base(w, h)
    for x, v in ((3, 0.0), (5, np.inf), (7, np.nan), (9, -1.0)):
        c["xv"][:, x, 3] = v
    c["reach"] = lambda n: not (n[:, [3, 5, 7, 9]] > F(N_CALL)).any() and (n[:, [2, 4, 6, 8, 10]] > F(N_CALL)).all()
    out["length_not_valid"] = c
    # a NaN and an infinity in a tap: D, V, n, P, N, A and the class of one history pixel each; and in the call's own Pv, P and N
    c = base(w, h)
    for i, (img, ch) in enumerate((("h0", 0), ("h0", 3), ("h2", 3), ("h2", 1), ("h1", 0), ("ha", 2), ("h1", 3))):
        c[img][1 + i, 9, ch] = np.nan
        c[img][1 + i, 20, ch] = np.inf
    c["xv"][2, 3, 1] = np.nan
    c["x2"][4, 3, 0] = np.nan
    c["x1"][6, 3, 2] = np.nan
    # (an infinite component of a tap's normal is the one thing the tests let through — N . N_q >= 0.9 holds for +inf — as temporal_merge does: row 5 is not asked)
    c["reach"] = lambda n: np.isfinite(n).all() and (n[[2, 4, 6], 3] == F(N_CALL)).all() and (n[1:8, 9] == F(N_CALL)).all() and (n[[1, 2, 3, 4, 6, 7], 20] == F(N_CALL)).all() and (n[:, 25] > F(N_CALL)).all()
    out["nan_and_infinity"] = c
    # no history at all
    c = base(w, h)
    c["have"] = 0
    c["reach"] = lambda n: (n == F(N_CALL)).all()
    out["no_history"] = c
    return out


def split(img):
    return np.ascontiguousarray(img[..., :3]), np.ascontiguousarray(img[..., 3])


def truth(case):
    """(Dm, Vm, n_out, followed, with_history) by tests/virtual_truth.py"""
    (D0, V0), (N, cls), (P, n), (A, _), (Pv, dist) = (split(case[k]) for k in ("x0", "x1", "x2", "xa", "xv"))
    hist = None
    if case["have"]:
        (hD, hV), (hN, hcls), (hP, hn), (hA, _) = (split(case[k]) for k in ("h0", "h1", "h2", "ha"))
        hist = dict(D=hD, V=hV, n=hn, N=hN, P=hP, A=hA, cls=hcls, cam=TT.camera(*case["cam"]))
    Dm, Vm, no = V.merge(D0, V0, n, N, P, A, cls, Pv, dist, hist, case["cap"])
    with np.errstate(all="ignore"):
        followed = cls >= F(2.0)
    return Dm, Vm, no, int(followed.sum()), int((followed & (no > n)).sum())
