"""The geometry kernels' inputs at the numeric edges of finite, accepted input, named once (not a test module): coordinates, matrices, weights and
deltas whose arithmetic underflows to denormals or zero, or overflows to inf (and from there to NaN), inside refit.hpp, pose.hpp, mesh.hpp, lbvh.hpp,
woop.hpp and tree_cost.hpp — and joint and target indices at the top of their 16 bits.  tests/test_geometry_edge_inputs.py holds on the CPU that every
rung reaches the branch it exists for (from the numpy truths' side only) and that the host twins equal the truths there; tests/test_gpu_geometry_edges.py
runs the rungs through the kernels.  Every scaling is done in binary64 and rounded to binary32 once.  The scenes are tests/test_gpu_pose.Small(257)
(T.soup(257, 3) with texture coordinates and material ids), M.grid(8, 6), M.fan(300), gentle(6) and M.entries_of(257, 3): 257 is one triangle past a
workgroup, the fan's apex is one lane's loop of 300 trips."""
import functools

import numpy as np

from tests import mesh_truth as M
from tests import morph_truth as MO
from tests import pose_truth as P
from tests.test_gpu_pose import gentle, small

F = np.float32
N_TRIS = 257
N_MATRICES = 6
N_TARGETS = 3
TINY = F(2.0 ** -149)        # the smallest denormal
MIN_NORMAL = F(2.0 ** -126)

# ---- the ladders: the exponents k of the factor 2^k ----
# coordinates (refit.hpp, woop.hpp, tree_cost.hpp, lbvh.hpp, ploc.hpp, presplit.hpp): -149 every coordinate is 0 or the smallest denormal (cell 0: exponent
# byte 0, or denormal: byte 1); -140, -126 denormal cells (byte 1, the division by 2^-126); -100 normal cells, areas that underflow to 0 (Cost() refuses);
# -64, 40 plain numbers whose areas are still finite; 64, 100 areas that overflow to inf; 124 extents near 2^127: the byte is clamped to 254
COORD_K = (-149, -140, -126, -100, -64, 0, 40, 64, 100, 124)
# meshes (mesh.hpp): face vectors and len2 go with 2^2k and 2^4k.  -75, -74 face vectors 0 or denormal; -64, -38 len2 0: nothing normalised; -37, -36 len2
# denormal and normalised (sqrtf and / on denormal operands); -31 the last denormal len2; 31 the last rung with every len2 finite; 32 some len2 inf; 33, 64
# every len2 inf or NaN: nothing normalised; 100 face vectors inf, inf - inf in the sums
MESH_K = (-75, -74, -64, -38, -37, -36, -31, 0, 31, 32, 33, 64, 100)
# matrices (pose.hpp): the cofactors go with 2^2k, len2 with 2^4k; the positions stay finite throughout
MATRIX_K = (-75, -38, -37, -36, -33, 0, 31, 32, 33, 63)
GIVEN_NORMAL_K = (-140, 120)         # given normals are used as given, whatever their length
REBUILD_K = (-149, -126, -100, -64, 40)
RAY_K = (-64, 0, 40, 64)
REFUSED_K = 60                       # node areas of about 2^129: every SAH cost overflows, every host builder refuses (the SBVH builder used not to return)
WEIGHT_RUNGS = ("denormal", "min_normal", "huge")
MORPH_RUNGS = ("underflow", "large", "overflow", "minus_zero", "denormal_weight")
INDEX_RUNGS = ("skin_top_joint", "morph_top_target")

# The rungs whose TRUTH has a NaN among its posed positions: there the refit's unions depend on their order (refit_min with a NaN), so only the records
# are compared.  Derived in tests/test_geometry_edge_inputs.py from the numpy truths, which must give exactly this list; no rung of the three ladders may
# be on it.  ("weights", "huge"): 3e38 times a matrix entry above 1.13 is inf, and inf * x + -inf * y is NaN.  ("morph", "overflow"): products w * d that
# are inf, of both signs, on one word
NAN_POSITIONS = (("weights", "huge", "skin"), ("morph", "overflow", "parts"), ("morph", "overflow", "skin"))


def scaled(a, k):
    """a * 2^k in binary64, rounded to binary32 once (inf where it does not fit)"""
    with np.errstate(over="ignore", under="ignore"):
        return (np.asarray(a, dtype=np.float64) * 2.0 ** k).astype(F)


# ---- coordinates ----
@functools.lru_cache(maxsize=None)
def soup(k):
    """Small(257).tris with the positions times 2^k; shared and never written"""
    t = np.array(small(N_TRIS).tris)
    t["p"] = scaled(t["p"], k)
    t.setflags(write=False)
    return t


# ---- meshes ----
MESHES = {"grid": lambda: M.grid(8, 6), "fan": lambda: M.fan(300)}


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(indices, positions) at k = 0"""
    idx, p = MESHES[name]()
    idx.setflags(write=False)
    p.setflags(write=False)
    return idx, p


@functools.lru_cache(maxsize=None)
def mesh_positions(name, k):
    p = scaled(mesh(name)[1], k)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def given_normals(name, k):
    n = scaled(M.some_normals(len(mesh(name)[1])), k)
    n.setflags(write=False)
    return n


# ---- matrices ----
@functools.lru_cache(maxsize=None)
def matrices(k):
    """gentle(6) with the 3x3 parts times 2^k; the translations stay"""
    m = np.array(gentle(N_MATRICES))
    m[:, :, :3] = scaled(m[:, :, :3], k)
    m.setflags(write=False)
    return m


def binding(kind, n=N_TRIS, nm=N_MATRICES):
    """parts_of / skin_of as tests/test_gpu_pose.binding_of gives them"""
    if kind == "parts":
        return {"parts": P.parts_of(n, nm)}
    j, w = P.skin_of(n, nm)
    return {"joints": j, "weights": w}


# ---- skin weights ----
def weight_rung(name):
    """skin_of(257, 6) with the vertices of every even triangle given the rung's weights in all four slots (joints in range there), the odd triangles as
    they are: both kinds side by side in every wave"""
    j, w = P.skin_of(N_TRIS, N_MATRICES)
    j, w = j.copy(), w.copy()
    even = np.arange(N_TRIS) % 2 == 0
    j[even] = np.random.RandomState(23).randint(0, N_MATRICES, size=j[even].shape)
    if name == "denormal":
        w[even] = TINY
    elif name == "min_normal":
        w[even] = MIN_NORMAL
    elif name == "huge":
        w[even] = 1.0
        w[even, :, 1] = 3e38
    else:
        raise KeyError(name)
    return {"joints": j, "weights": w}


# ---- morph layers ----
def morph_rung(name):
    """(entries, weights) on M.entries_of(257, 3)"""
    tri, tgt, d = MO.entries_of(N_TRIS, N_TARGETS)
    if name == "underflow":        # every product is a denormal or 0
        return (tri, tgt, scaled(d, -40)), np.full(N_TARGETS, 2.0 ** -100, F)
    if name == "large":            # products up to 2^126.3 (the largest |d| is 0.44): the largest morphed and posed words that stay finite
        return (tri, tgt, scaled(d, 27)), np.full(N_TARGETS, 2.0 ** 100, F)
    if name == "overflow":         # every product with |d| >= 2^-3 is inf: inf + -inf in the sums of one word, NaN positions
        return (tri, tgt, scaled(d, 31)), np.full(N_TARGETS, 2.0 ** 100, F)
    if name == "minus_zero":       # == 0: skipped, the deltas never read
        return (tri, tgt, d), np.full(N_TARGETS, -0.0, F)
    if name == "denormal_weight":  # != 0: taken.  Deltas of +-3e38, so that a product is +-4.2e-7 and shows in words of magnitude below 4
        return (tri, tgt, np.where(d < 0, F(-3e38), F(3e38)).astype(F)), np.full(N_TARGETS, TINY, F)
    raise KeyError(name)


# ---- indices at the top of their 16 bits ----
TOP, HIGH = 65535, 40000  # HIGH >= 32768: its sign bit as an int16


@functools.lru_cache(maxsize=None)
def many_matrices():
    """65 536 matrices: gentle(6) over and over, 65 535 and 40 000 two of their own — unlike 32 767, 7 232 (HIGH - 32 768) and -1 % 6"""
    m = np.array(np.resize(gentle(N_MATRICES), (65536, 3, 4)))
    m[TOP] = P.rotation((1.0, -2.0, 0.5), 61.0, (-0.75, 0.5, 0.25))
    m[HIGH] = P.rotation((-0.4, 0.3, 1.0), -48.0, (0.3, 0.9, -0.6))
    m.setflags(write=False)
    return m


def index_rung(name):
    """skin_top_joint: (binding, matrices) — slot s of every vertex of triangle 4 s + 1 names joint 65 535 and of triangle 4 s + 2 joint 40 000, weight 0.5,
    beside what skin_of gave the other slots.  morph_top_target: (parts binding, matrices, entries, weights) — the targets 0, 1, 2 of entries_of(257, 3)
    renamed 0, 40 000 and 65 535, all three with a weight"""
    if name == "skin_top_joint":
        j, w = P.skin_of(N_TRIS, 65536)
        j, w = j.copy(), w.copy()
        for s in range(4):
            j[4 * s + 1, :, s], w[4 * s + 1, :, s] = TOP, 0.5
            j[4 * s + 2, :, s], w[4 * s + 2, :, s] = HIGH, 0.5
        return {"joints": j, "weights": w}, many_matrices()
    if name == "morph_top_target":
        tri, tgt, d = MO.entries_of(N_TRIS, N_TARGETS)
        tgt = np.array([0, HIGH, TOP], np.int32)[tgt]
        w = np.zeros(65536, F)
        w[[0, HIGH, TOP]] = (-0.75, 0.5, 1.25)
        return binding("parts"), matrices(0), (tri, tgt, d), w
    raise KeyError(name)


# ---- rays ----
N_RAYS = 2048


def rays(k):
    """T.rays_in_box(soup(k), 1024) with tmin scaled like the scene — of which the oracle hits on 36 at k = 0, and on at most 41 with any of the seeds
    0 .. 199: 257 small triangles in a box of 20^3 — and 1024 more from one point outside the scene at points inside the triangles (as
    tests/test_gpu_set_triangles.aimed_rays aims them at k = 0), origin and tmin scaled, the directions as they are"""
    from tests import refit_truth as T
    from tests.test_gpu_set_triangles import aimed_rays
    r = T.rays_in_box(soup(k), 1024)
    r[:, 3] = scaled(r[:, 3], k)
    aimed = aimed_rays(soup(0), 1024)
    aimed[:, :4] = scaled(aimed[:, :4], k)
    return np.concatenate([r, aimed])
