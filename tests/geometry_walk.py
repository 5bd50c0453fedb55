"""A context's geometry calls in random order (no GPU here): the vocabulary of operations, a host model of what a context holds after each, and the
generator of the walks that tests/test_geometry_walk.py (CPU) and tests/test_gpu_geometry_walk.py (-m gpu) run.

An operation is (kind, arg): a name of GEOMETRY, DISTURBANCES or REFUSALS and a small integer from which the model draws everything else (positions,
matrices, parts, counts), so that a list of operations prints short and replay() of the printed list makes the same arrays again.

The model is plain Python over host arrays and advances by what the suite already holds true on the CPU: tests/pose_truth.py, morph_truth.py and
mesh_truth.py for records, adypt_bvh_refit for a refit, WideBVH.BuildLinear / BuildPLOC for a rebuild and for new triangles, WideBVH.Cost for the
numbers a policy reports.  The lifetime rules are README's (Moving geometry, Posing, Morph targets, Meshes), each written once, in Model.apply:
a rebuild keeps bindings; SetTriangles drops all three; an update writes posed records and never the rest pose; a new bind captures the records as they
are; BindParts / BindSkin / UnbindPose drop the morph layer; the last writer of the records stands; a refit drops a split tree's reference boxes; the
policy's reference cost is taken at the first GetTreeCost() or policy call after the upload or a rebuild, on the tree as it is then."""
import numpy as np

from adypt_amd import api, _native as N
from oracle import oracle_py as O
from tests import mesh_truth as ME
from tests import morph_truth as MO
from tests import pose_truth as P
from tests import refit_truth as T
from tests.test_refit_definition import lib_refit

COUNTS = (1, 5, 255, 256, 257, 554, 3000)  # 256: a workgroup of k_pack_triangles, k_pose and the mesh kernels
START_COUNTS = (5, 255, 256)               # a walk begins low, so that "above every earlier count" has somewhere to go
OTHER_RADIUS = 3
N_RAYS = 4096

GEOMETRY = ("update_all", "update_range", "update_rebuild", "update_keep", "rebuild_linear", "rebuild_ploc", "rebuild_split", "set_below", "set_equal",
            "set_above", "bind_parts", "bind_skin", "pose", "unbind_pose", "bind_morph", "pose_morph", "unbind_morph", "bind_mesh", "pose_vertices",
            "unbind_mesh", "pose_policy", "pose_vertices_policy")
# they change no geometry and leave derived state behind: an image and a primary-hit cache, frames parked ahead, noise moments and frozen blocks, the
# denoiser's history and motion snapshot, the measured reference cost, a forgotten started frame
DISTURBANCES = ("trace", "lookahead", "adaptive", "denoise", "tree_cost", "trace_rays")
# drawn on purpose; (pose and pose_vertices after a call that dropped their binding come about as pairs of GEOMETRY as well)
REFUSALS = ("refuse_pose", "refuse_pose_vertices", "refuse_update_range", "refuse_bind")

# they move no triangle and leave the accumulation alone; every other kind leaves the context as Reset() does
KEEP_THE_IMAGE = ("bind_parts", "bind_skin", "unbind_pose", "bind_morph", "unbind_morph", "bind_mesh", "unbind_mesh")
NEEDS_POSE = ("pose", "pose_policy", "unbind_pose", "bind_morph")
NEEDS_MORPH = ("pose_morph", "unbind_morph")
NEEDS_MESH = ("pose_vertices", "pose_vertices_policy", "unbind_mesh")
NO_POSE = {"kind": 0, "n_matrices": 0, "n_tris": 0}
NO_MORPH = {"n_targets": 0, "n_entries": 0, "n_tris_touched": 0}
NO_MESH = {"n_vertices": 0, "n_tris": 0, "max_valence": 0}


# ---- inputs, each from (the triangles as they are, a small integer) ----
def triangles_of(n, seed):
    """A soup with texture coordinates and material ids (0, and -1 on every third) that every call but SetTriangles must keep.  The camera of the walks
    stands in the middle of tests/refit_truth.soup and sees a third of 3 000 triangles, but of five it sees none: up to 257 the triangles stand in
    front of it instead, 4 to 12 units away, 1.5 times the size (4 times up to five), so that the image of every step shows some."""
    t = T.soup(n, 100 + seed)
    if n <= 257:
        rs = np.random.RandomState(1000 + seed)
        view = np.asarray(api.camera_matrices(60.0, 30.0, -10.0, 32, 18)[1], dtype=np.float64).reshape(4, 4)[:3, :3]  # rows: right, up, backwards
        d = rs.uniform(4.0, 12.0, size=n)
        centre = -view[2] * d[:, None] + view[0] * (rs.uniform(-0.45, 0.45, size=n) * d)[:, None] + view[1] * (rs.uniform(-0.25, 0.25, size=n) * d)[:, None]
        p = t["p"].astype(np.float64)
        t["p"] = ((p - p.mean(axis=1, keepdims=True)) * (4.0 if n <= 5 else 1.5) + centre[:, None, :]).astype(np.float32)
    t["tc"] = np.random.RandomState(seed).uniform(size=t["tc"].shape).astype(np.float32)
    t["matid"] = np.where(np.arange(n) % 3 == 2, -1, 0)
    return t


def moved(tris, arg):
    """gentle: the wave of tests/refit_truth.py or a jitter, so that triangles stay triangles"""
    return T.wave(tris) if arg % 3 == 0 else T.jitter(tris, 11 + arg)


def tilted(tris, arg):
    n = tris["n"].astype(np.float64) + np.array([0.3, -0.2, 0.1]) * (1 + arg % 2)
    return (n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-20)).astype(np.float32)


def range_of(n, arg):
    first = (n // 3, 0, n - 1)[arg % 3]
    return first, min(n - first, n // 2 + 1)


def matrices_of(nm, arg):
    """nm gentle affine maps (tests/pose_truth.matrix_set behind its four fixed ones): a rotation, scales in [0.8, 1.25], a small translation"""
    return np.ascontiguousarray(P.matrix_set(nm + 4, 3 + arg)[4:])


def skin_of(n, nm, arg):
    """tests/pose_truth.skin_of without a vertex that follows no joint: every triangle stays one"""
    j, w = P.skin_of(n, nm, 9 + arg)
    none = (w == 0).all(axis=-1)
    w[none, 0], j[none, 0] = 1.0, min(1, nm - 1)
    return j, w


AIM_FROM = np.array([(37.0, 41.0, 43.0), (-37.0, 41.0, 43.0), (37.0, -41.0, 43.0), (37.0, 41.0, -43.0)]) / np.linalg.norm((37.0, 41.0, 43.0))
AIM_COS = 0.2
AIM_SEED = 5


def aimed_rays(tris, n, seed=None):
    """Rays at points inside the triangles, ray i at triangle i % len(tris), as tests/test_gpu_set_triangles.py aims them from (37, 41, 43) — with two differences.
    The point lies in that direction two diagonals of the triangles' box from its centre, which is where (37, 41, 43) is for the soups of that
    test: a walk takes its triangles elsewhere, and one triangle seen from a hundred times its size away has a t whose binary32 spacing is more
    than the 1e-5 of the diagonal that tests/helpers.check_against_fp64_truth holds t to.  And a
    triangle that this point sees nearly edge-on (|cos| of the angle between its plane's normal and the ray below AIM_COS) is aimed at from the first
    of three mirror images of the point that sees it better.  A ray from the box meets an edge-on triangle in proportion to the little area it
    shows; a ray aimed at one meets it always, and there binary32 cannot give t: the intersection's error along the ray is its error across the
    plane, a few ulp of coordinates of 40 or so (some 1e-6 of the diagonal), divided by that cosine, and the t of tests/helpers.check_against_fp64_truth
    must hold to 1e-5 of the diagonal.  At 0.2 the quotient stays below it; no normal is below 0.2 from all four points."""
    rs = np.random.RandomState(AIM_SEED if seed is None else seed)
    w = rs.dirichlet((2.0, 2.0, 2.0), size=n)
    at = np.arange(n) % len(tris)
    p = tris["p"].astype(np.float64)
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    lo, hi = p.reshape(-1, 3).min(axis=0), p.reshape(-1, 3).max(axis=0)
    points = ((lo + hi) / 2 + 2 * np.linalg.norm(hi - lo) * AIM_FROM).astype(np.float32).astype(np.float64)
    d = p.mean(axis=1)[:, None, :] - points[None, :, :]  # [triangle, point, axis]
    cos = np.abs((d * normal[:, None, :]).sum(-1)) / np.maximum(np.linalg.norm(d, axis=-1) * np.linalg.norm(normal, axis=-1)[:, None], 1e-300)
    good = cos >= AIM_COS
    origin = points[np.where(good.any(axis=1), good.argmax(axis=1), cos.argmax(axis=1))][at]
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3], rays[:, 3] = origin, 1e-4
    rays[:, 4:7] = (p[at] * w[:, :, None]).sum(axis=1) - origin
    return rays


EDGE_ON = 0.05


def edge_on(tris, rays):
    """Which rays hit, in binary64 and with a hundredth of the triangle to spare on every side, a triangle whose plane they meet at a cosine below
    EDGE_ON.  There binary32 cannot give t to the 1e-5 of the diagonal that check_against_fp64_truth holds every reported hit to (see aimed_rays: a
    few 1e-7 of the diagonal over the cosine; the walks' soups gave 1e-5 to 9e-5 at cosines of 0.001 to 0.002), whichever implementation computes it."""
    p = tris["p"].astype(np.float64)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    normal = np.cross(e1, e2)
    normal /= np.maximum(np.linalg.norm(normal, axis=1, keepdims=True), 1e-300)
    o, d = rays[:, :3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    ray, tri = np.nonzero(np.abs(d @ normal.T) < EDGE_ON)  # (the few pairs that are edge-on at all)
    with np.errstate(divide="ignore", invalid="ignore"):  # Moeller and Trumbore; a ray in the plane itself divides by 0 and counts as a hit
        h = np.cross(d[ray], e2[tri])
        a = (e1[tri] * h).sum(-1)
        s = o[ray] - p[tri, 0]
        u = (s * h).sum(-1) / a
        q = np.cross(s, e1[tri])
        v = (d[ray] * q).sum(-1) / a
        t = (e2[tri] * q).sum(-1) / a
        hit = ~((u < -0.01) | (v < -0.01) | (u + v > 1.01) | (t < 0))
    out = np.zeros(len(rays), dtype=bool)
    out[ray[hit]] = True
    return out


def rays_of(tris):
    """A step's 4096 rays: half from the scene's box, half aimed at the triangles; below five triangles box rays find nothing, so all are aimed.  A ray
    that meets a triangle edge-on gives its place to the ray in front of it."""
    rays = aimed_rays(tris, N_RAYS) if len(tris) < 5 else np.concatenate([T.rays_in_box(tris, N_RAYS // 2), aimed_rays(tris, N_RAYS // 2)])
    keep = np.nonzero(~edge_on(tris, rays))[0]
    return rays[keep[np.clip(np.searchsorted(keep, np.arange(len(rays)), side="right") - 1, 0, None)]]


def least_hits(n_tris):
    """the least number of a step's rays that the oracle must reach.  From five triangles on: 1500 of 4096.  Below, every ray is aimed at a point
    inside a triangle and hits unless it grazes an edge: all but 96, the allowance tests/test_gpu_set_triangles.py gives such rays (4000 of 4096)."""
    return 1500 if n_tris >= 5 else 4000


class Case:
    """what tracer() of tests/test_gpu_refit.py asks of a case: the triangles a walk starts from, with the SBVH tree a context is created on"""

    def __init__(self, tris):
        self.tris = tris
        self.scene = api.Scene.FromArrays(tris, T.soup_material())
        self.ip, self.iv = api.camera_matrices(60.0, 30.0, -10.0, 32, 18)
        self.pos = np.zeros(3, np.float32)
        self._b = api.WideBVH()
        self._b.Build(self.scene, api.InstanceConfig().bvh_params())

    def bvh(self, depth=48):
        return self._b


class Step:
    """one operation as the model saw it: the call to make, what it must answer, and everything the context must hold afterwards (never written)"""

    def __init__(self, op, category, call, refused, answer, model):
        self.op, self.category, self.call, self.refused, self.answer = op, category, call, refused, answer
        self.tris, self.nodes, self.tri_indices, self.woop, self.ref_boxes = model.tris, model.nodes, model.tri_indices, model.woop, model.ref_boxes
        self.info, self.cost = model.info, model.cost
        self.pose, self.morph, self.mesh = model.pose_binding(), model.morph_binding(), model.mesh_binding()
        self._rays = None

    def rays(self):
        """rays_of(self.tris), made once"""
        if self._rays is None:
            self._rays = _frozen(rays_of(self.tris))
        return self._rays


class Model:
    def __init__(self, start):
        self.mats = T.soup_material()
        self.case = Case(_frozen(triangles_of(START_COUNTS[start % len(START_COUNTS)], start)))
        self.tris = self.case.tris
        self.largest = len(self.tris)
        self.previous_count = None  # the count before the last SetTriangles that changed it
        self._adopt(self.case.bvh(), None)
        self.binding = self.rest = self.layer = self.mesh = None

    # -- the tree --
    def _adopt(self, b, info):
        """a tree as built: the policy's reference cost is stale until it is next asked for"""
        self.nodes, self.tri_indices = _frozen(np.array(b.nodes)), _frozen(np.array(b.tri_indices))
        self.ref_boxes = _frozen(np.array(b.ref_boxes)) if len(b.ref_boxes) else None
        self.woop = api.woop_matrices(self.tris, self.tri_indices)
        self.info = info
        self.cost, self.built = b.Cost(), None

    def _build(self, method, radius=8, budget=0.0):
        b = api.WideBVH()
        s = api.Scene.FromArrays(self.tris, self.mats)
        if method == "linear":
            b.BuildLinear(s, api.InstanceConfig().bvh_params())
        else:
            b.BuildPLOC(s, api.InstanceConfig().bvh_params(), radius, budget)
        info = {"n_nodes": len(b.nodes) // 80, "n_refs": len(b.tri_indices), "levels": int(T.depths(np.ascontiguousarray(b.nodes).view(O.NODE_DT)).max()) + 1}
        self._adopt(b, info)
        return info

    def _refit(self):
        """the triangles are self.tris now: the nodes follow, the references bound whole triangles from here on"""
        r, nodes = lib_refit(self.nodes, self.tri_indices, self.tris)
        assert r == N.ADYPT_OK
        self.nodes, self.ref_boxes = _frozen(nodes), None
        self.woop = api.woop_matrices(self.tris, self.tri_indices)
        self.cost = _cost(self.nodes)

    def ask_cost(self):
        """GetTreeCost(), or the beginning of a policy call: a stale reference cost is taken now, on the tree as it is (README, Refit or rebuild)"""
        if self.built is None:
            self.built = self.cost
        return self.cost

    def _under_policy(self, above, method):
        """what adypt_update_triangles_auto and its kin answer around the refit that has just been made (ask_cost() stood in front of it)"""
        out = {"built": self.built, "refitted": self.cost, "now": self.cost, "rebuilt": 0, "rebuild": None}
        if out["refitted"]["cost"] > above * out["built"]["cost"]:
            out["rebuild"] = self._build(method)
            out["now"], out["rebuilt"] = self.ask_cost(), 1  # (the new tree's, which is the reference from here on)
        return out

    def _write(self, tris):
        self.tris = _frozen(tris)

    # -- the bindings, as the getters give them (without device_bytes) --
    def pose_binding(self):
        return dict(NO_POSE) if self.binding is None else {"kind": 1 if "parts" in self.binding else 2, "n_matrices": self.nm, "n_tris": len(self.rest)}

    def morph_binding(self):
        if self.layer is None:
            return dict(NO_MORPH)
        return {"n_targets": self.nt, "n_entries": len(self.layer[0]), "n_tris_touched": len(np.unique(self.layer[0]))}

    def mesh_binding(self):
        if self.mesh is None:
            return dict(NO_MESH)
        idx, pos = self.mesh
        return {"n_vertices": len(pos), "n_tris": len(idx), "max_valence": int(np.bincount(idx.ravel()).max())}

    # -- one operation --
    def apply(self, op):
        kind, arg = op
        category = "geometry" if kind in GEOMETRY else "disturbance" if kind in DISTURBANCES else "refusal"
        assert category != "refusal" or kind in REFUSALS, kind
        call, refused, answer = getattr(self, "_" + kind)(arg) if category != "disturbance" else ((kind, (arg,), {}), None, None)
        if kind == "tree_cost" or (category == "geometry" and refused is None):
            self.ask_cost()  # (the walk asks for GetTreeCost() behind every geometry call that was made, and the disturbance is that question)
        return Step(op, category, call, refused, answer, self)

    def _update_all(self, arg):
        t = moved(self.tris, arg)
        self._write(t)
        self._refit()
        return ("UpdateTriangles", (0, t["p"].reshape(-1, 9)), {}), None, None

    def _update_range(self, arg):
        n = len(self.tris)
        first, count = range_of(n, arg)
        sl, with_normals = slice(first, first + count), arg % 2 == 1
        m, t = moved(self.tris, arg), np.array(self.tris)
        t["p"][sl] = m["p"][sl]
        nrm = None
        if with_normals:
            t["n"][sl] = tilted(self.tris, arg)[sl]
            nrm = t["n"][sl].reshape(-1, 9)
        self._write(t)
        self._refit()
        return ("UpdateTriangles", (first, t["p"][sl].reshape(-1, 9), nrm), {}), None, None

    def _update_policy(self, arg, above):
        self.ask_cost()
        t = moved(self.tris, arg)
        self._write(t)
        self._refit()
        method = ("ploc", "linear")[arg % 2]
        return ("UpdateTriangles", (0, t["p"].reshape(-1, 9)), dict(rebuild_above=above, method=method)), None, self._under_policy(above, method)

    def _update_rebuild(self, arg):
        return self._update_policy(arg, 0.0)

    def _update_keep(self, arg):
        return self._update_policy(arg, 1e9)

    def _rebuild_linear(self, arg):
        return ("RebuildBVH", (), dict(method="linear")), None, self._build("linear")

    def _rebuild_ploc(self, arg):
        radius = (8, OTHER_RADIUS)[arg % 2]
        return ("RebuildBVH", (), dict(method="ploc", radius=radius)), None, self._build("ploc", radius)

    def _rebuild_split(self, arg):
        return ("RebuildBVH", (), dict(method="ploc", split_budget=0.3)), None, self._build("ploc", 8, 0.3)

    def _set(self, n, arg):
        if n != len(self.tris):
            self.previous_count = len(self.tris)
        self._write(triangles_of(n, 31 * arg + n))
        self.largest = max(self.largest, n)
        self.binding = self.rest = self.layer = self.mesh = None
        method = ("ploc", "linear")[arg % 2]
        return ("SetTriangles", (self.tris,), dict(method=method)), None, self._build(method)

    def _set_below(self, arg):
        below = [c for c in COUNTS if c < len(self.tris)] or [1]  # (at one triangle: one again)
        return self._set(below[arg % len(below)], arg)

    def _set_equal(self, arg):
        return self._set(len(self.tris), arg)

    def _set_above(self, arg):
        """above every earlier count; once a walk has been at 3 000, that count again"""
        above = [c for c in COUNTS if c > self.largest] or [COUNTS[-1]]
        return self._set(above[arg % len(above)], arg)

    def _bind(self, binding, nm):
        self.binding, self.nm, self.rest, self.layer = binding, nm, self.tris, None  # (captures the records as they are; the layer was the old rest pose's)

    def _bind_parts(self, arg):
        nm = (1, 3, 6)[arg % 3]
        parts = P.parts_of(len(self.tris), nm, 5 + arg)
        self._bind({"parts": parts}, nm)
        return ("BindParts", (parts, nm), {}), None, None

    def _bind_skin(self, arg):
        nm = (3, 6)[arg % 2]
        j, w = skin_of(len(self.tris), nm, arg)
        self._bind({"joints": j, "weights": w}, nm)
        return ("BindSkin", (j, w, nm), {}), None, None

    def _posed(self, arg, morphed):
        mats = matrices_of(self.nm, arg)
        if morphed:
            w = MO.weights_of(self.nt, 17 + arg)
            return mats, w, MO.pose(self.rest, mats, self.layer, w, **self.binding)
        return mats, None, P.pose(self.rest, mats, **self.binding)

    def _pose(self, arg, above=None):
        if self.binding is None:
            return ("Pose", (matrices_of(3, arg),), {}), N.E_STATE, None
        mats, _, t = self._posed(arg, False)
        if above is not None:
            self.ask_cost()
        self._write(t)
        self._refit()
        if above is None:
            return ("Pose", (mats,), {}), None, None
        return ("Pose", (mats,), dict(rebuild_above=above)), None, self._under_policy(above, "ploc")

    def _pose_policy(self, arg):
        return self._pose(arg, (0.0, 1e9)[arg % 2])

    def _unbind_pose(self, arg):
        self.binding = self.rest = self.layer = None
        return ("UnbindPose", (), {}), None, None

    def _bind_morph(self, arg):
        nt = (1, 3)[arg % 2]
        entries = MO.entries_of(len(self.tris), nt, 13 + arg)
        if self.binding is None:
            return ("BindMorph", entries + (nt,), {}), N.E_STATE, None
        self.layer, self.nt = entries, nt
        return ("BindMorph", entries + (nt,), {}), None, None

    def _pose_morph(self, arg):
        if self.binding is None:
            return ("Pose", (matrices_of(3, arg),), dict(morph_weights=MO.weights_of(3, 17 + arg))), N.E_STATE, None
        if self.layer is None:  # weights without a layer
            return ("Pose", (matrices_of(self.nm, arg),), dict(morph_weights=MO.weights_of(3, 17 + arg))), N.E_INVALID, None
        mats, w, t = self._posed(arg, True)
        self._write(t)
        self._refit()
        return ("Pose", (mats,), dict(morph_weights=w)), None, None

    def _unbind_morph(self, arg):
        self.layer = None
        return ("UnbindMorph", (), {}), None, None

    def _bind_mesh(self, arg):
        idx, pos, _ = api.weld_triangles(self.tris)
        self.mesh = (idx, pos)  # (no rest pose is captured: the vertex positions here are what the poses below start from)
        return ("BindMesh", (idx, len(pos)), {}), None, None

    def _pose_vertices(self, arg, above=None):
        if self.mesh is None:
            return ("PoseVertices", (np.zeros((3, 3), np.float32),), {}), N.E_STATE, None
        idx, rest = self.mesh
        pos = ME.deform(rest, 1 + arg % 3)
        given = ME.some_normals(len(pos), 2 + arg) if arg % 2 == 1 else None
        if above is not None:
            self.ask_cost()
        self._write(ME.triangles(self.tris, idx, pos, given))
        self._refit()
        if above is None:
            return ("PoseVertices", (pos, given), {}), None, None
        return ("PoseVertices", (pos, given), dict(rebuild_above=above, method="ploc", radius=8)), None, self._under_policy(above, "ploc")

    def _pose_vertices_policy(self, arg):
        return self._pose_vertices(arg, (0.0, 1e9)[arg // 2 % 2])

    def _unbind_mesh(self, arg):
        self.mesh = None
        return ("UnbindMesh", (), {}), None, None

    # -- refused on purpose: nothing changes --
    def _refuse_pose(self, arg):
        assert self.binding is None
        return ("Pose", (matrices_of(3, arg),), {}), N.E_STATE, None

    def _refuse_pose_vertices(self, arg):
        assert self.mesh is None
        return ("PoseVertices", (np.zeros((3 * len(self.tris), 3), np.float32),), {}), N.E_STATE, None

    def _old_count(self):
        assert self.previous_count not in (None, len(self.tris))
        return self.previous_count

    def _refuse_update_range(self, arg):
        old = self._old_count()
        first = 0 if old > len(self.tris) else len(self.tris) + 1  # a range of the old count, or one that begins past the new
        return ("UpdateTriangles", (first, np.zeros((old - first if old > first else 1, 9), np.float32)), {}), N.E_INVALID, None

    def _refuse_bind(self, arg):
        old = self._old_count()
        if arg % 3 == 0:
            return ("BindParts", (np.zeros(old, np.int32), 1), {}), N.E_INVALID, None
        if arg % 3 == 1:
            j, w = skin_of(old, 3, arg)
            return ("BindSkin", (j, w, 3), {}), N.E_INVALID, None
        return ("BindMesh", (np.arange(3 * old, dtype=np.int32).reshape(-1, 3), 3 * old), {}), N.E_INVALID, None


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _cost(nodes):
    b = api.WideBVH()
    b.nodes = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    return b.Cost()


# ---- the generator: symbols only, no arrays ----
class _Sketch:
    """what the generator must know of a context to keep a prefix legal"""

    def __init__(self, start):
        self.count = self.largest = START_COUNTS[start % len(START_COUNTS)]
        self.previous = None
        self.pose = self.morph = self.mesh = False

    def prerequisites(self, kind, rs):
        out = []
        if kind == "set_below" and self.count == 1:
            out.append("set_above")
        if kind in NEEDS_POSE + NEEDS_MORPH and not self.pose:
            out.append(("bind_parts", "bind_skin")[rs.randint(2)])
        if kind in NEEDS_MORPH and not self.morph:
            out.append("bind_morph")
        if kind in NEEDS_MESH and not self.mesh:
            out.append("bind_mesh")
        return out

    def after(self, kind, arg):
        if kind.startswith("set_"):
            n = self.count
            if kind == "set_below":
                below = [c for c in COUNTS if c < n] or [1]
                n = below[arg % len(below)]
            elif kind == "set_above":
                above = [c for c in COUNTS if c > self.largest] or [COUNTS[-1]]
                n = above[arg % len(above)]
            if n != self.count:
                self.previous = self.count
            self.count, self.largest = n, max(self.largest, n)
            self.pose = self.morph = self.mesh = False
        elif kind in ("bind_parts", "bind_skin"):
            self.pose, self.morph = True, False
        elif kind == "unbind_pose":
            self.pose = self.morph = False
        elif kind == "bind_morph":
            self.morph = self.pose
        elif kind == "unbind_morph":
            self.morph = False
        elif kind == "bind_mesh":
            self.mesh = True
        elif kind == "unbind_mesh":
            self.mesh = False

    def refused(self, kind):
        """whether the context must refuse this kind now"""
        return (kind in ("pose", "pose_policy", "bind_morph", "pose_morph") and not self.pose) or (kind == "pose_morph" and not self.morph) or \
            (kind in ("pose_vertices", "pose_vertices_policy") and not self.mesh)

    def takes_away(self, a, b):
        """whether a leaves the context without what b needs, whatever stood before a"""
        return (a.startswith("set_") and b in NEEDS_POSE + NEEDS_MORPH + NEEDS_MESH) or (a == "unbind_pose" and b in NEEDS_POSE + NEEDS_MORPH) or \
            (a in ("bind_parts", "bind_skin", "unbind_morph") and b in NEEDS_MORPH) or (a == "unbind_mesh" and b in NEEDS_MESH)

    def refusals(self):
        """the refusals that can be drawn now"""
        out = []
        if not self.pose:
            out.append("refuse_pose")
        if not self.mesh:
            out.append("refuse_pose_vertices")
        if self.previous not in (None, self.count):
            out += ["refuse_update_range", "refuse_bind"]
        return out


_PLANS = {}


def walks(n_steps=24):
    """All committed walks, each a list of (kind, arg) of about n_steps geometry operations.  One seeded shuffle of all ordered pairs of GEOMETRY is
    walked through from its beginning: a walk takes the next pair that is still open and begins with its last operation (one more step), else the first
    open one (two, and what they need in front: a bind before a pose), until it has n_steps; the next walk goes on where it stopped, and the last one
    closes the list.  So every ordered pair stands somewhere, its two operations next to each other with nothing but disturbances and refused calls
    between them (they change no geometry).  Where the first of a pair takes away what the second needs (SetTriangles, then Pose), the second is made
    all the same and must be refused.  In front of an operation goes a disturbance until its kind has stood behind every one of DISTURBANCES, and a
    refusal of REFUSALS from time to time, where the state allows one."""
    if n_steps in _PLANS:
        return _PLANS[n_steps]
    rs = np.random.RandomState(20240)
    todo = [(a, b) for a in GEOMETRY for b in GEOMETRY]
    rs.shuffle(todo)
    behind = {(d, k) for d in DISTURBANCES for k in GEOMETRY}  # (disturbance, the kind directly behind it) still to come
    out = []
    while todo:
        sketch, ops, last, n = _Sketch(len(out)), [], None, 0

        def emit(kind):
            nonlocal last, n
            arg = int(rs.randint(0, 12))
            refusals = sketch.refusals()
            if refusals and rs.randint(4) == 0:
                ops.append((refusals[rs.randint(len(refusals))], int(rs.randint(0, 12))))
            for d in DISTURBANCES:
                if (d, kind) in behind:
                    behind.discard((d, kind))
                    ops.append((d, 1 + int(rs.randint(3))))
                    break
            ops.append((kind, arg))
            if last is not None and (last, kind) in todo:
                todo.remove((last, kind))
            n += 1
            if sketch.refused(kind):  # (it changes nothing: the next operation stands behind `last` still)
                assert sketch.takes_away(last, kind), (last, kind)
                return
            sketch.after(kind, arg)
            last = kind

        while todo and n < n_steps:
            chained = [p for p in todo if p[0] == last]
            a, b = chained[0] if chained else todo[0]
            if not chained:
                for k in sketch.prerequisites(a, rs) + [a]:
                    emit(k)
            need = [] if sketch.takes_away(a, b) else sketch.prerequisites(b, rs)
            if need:  # (what b needs would stand between a and b: it goes in front of a, which is made once more)
                for k in need + [a]:
                    emit(k)
            emit(b)
        out.append(ops)
    _PLANS[n_steps] = out
    return out


def walk(seed, n_steps=24):
    return walks(n_steps)[seed]


SEEDS = tuple(range(len(walks())))

_replayed = {}


def replay(ops, start=0):
    """The model's Steps of an explicit list of (kind, arg), on the triangles that walk `start` begins with; ([initial Step] + one per operation).  A
    failure of a walk prints its list up to the failing step in this form."""
    m = Model(start)
    steps = [Step(("create", start), "create", None, None, None, m)]
    for op in ops:
        steps.append(m.apply(tuple(op)))
        if steps[-1].tris is steps[-2].tris:
            steps[-1].rays = steps[-2].rays  # (the same triangles: the same rays, made once)
    return m.case, steps


def steps_of(seed):
    """replay(walk(seed), seed), made once; the last few are kept"""
    if seed not in _replayed:
        while len(_replayed) >= 4:
            _replayed.pop(next(iter(_replayed)))
        _replayed[seed] = replay(walk(seed), seed)
    return _replayed[seed]
