"""Host-side mirror of the reference's interface for the hot path, on top of the C-ABI.

Names and call order follow the reference so that tests read like its own call sites:

    InstanceConfig.LoadFromFile / GetJson / SaveToFile        src/InstanceConfig.cpp:10-210
    Scene.LoadFromFile                                        src/Util/Scene.cpp:9-136
    WideBVH.LoadFromFile / SaveToFile, build_bvh()            src/BVH/WideBVH.cpp:9-66, src/Instance.cpp:20-32
    Camera.GetInvProjection / GetInvView                      src/Tracer/Camera.cpp:13-23 (+ inverses of SetCamera)
    HipScene.Initialize(scene, bvh)                           OglScene::Initialize, src/Tracer/OglScene.hpp:43
    HipPathTracer.Initialize / SetCamera / Trace / SaveResult / GetSPP
                                                              OglPathTracer, src/Tracer/OglPathTracer.hpp:66-82
    Instance.InitializeFromFile / Update                      src/Instance.cpp:10-69

Everything numeric happens in libadypt_hip.so; this module only marshals numpy arrays.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N

NODE_BYTES, TRI_BYTES, MAT_BYTES = 80, 100, 64
HIT_DT = np.dtype([("ref_idx", "<i4"), ("tri_id", "<i4"), ("u", "<f4"), ("v", "<f4"), ("t", "<f4"),
                   ("nodes", "<u4"), ("tris", "<u4"), ("hash", "<u4"), ("max_depth", "<u4")])


def _bytes_view(ptr: int, n: int) -> np.ndarray:
    if n == 0:
        return np.zeros(0, dtype=np.uint8)
    return np.frombuffer((C.c_char * n).from_address(ptr), dtype=np.uint8).copy()


# ---------------------------------------------------------------------------------------------------------------
class InstanceConfig:
    """`.config` JSON <-> struct (src/InstanceConfig.hpp:12-48)."""

    def __init__(self) -> None:
        self.c = N.Config()
        self.SetDefault()

    def SetDefault(self) -> None:
        N.lib.adypt_config_default(C.byref(self.c))

    def LoadFromFile(self, filename: str) -> bool:
        return N.lib.adypt_config_load(filename.encode(), C.byref(self.c)) == N.ADYPT_OK

    def Parse(self, text: str) -> bool:
        return N.lib.adypt_config_parse(text.encode(), C.byref(self.c)) == N.ADYPT_OK

    def GetJson(self) -> str:
        n = N.lib.adypt_config_json(C.byref(self.c), None, 0)
        buf = C.create_string_buffer(n)
        N.lib.adypt_config_json(C.byref(self.c), buf, n)
        return buf.value.decode()

    def SaveToFile(self, filename: str) -> bool:
        return N.lib.adypt_config_save(filename.encode(), C.byref(self.c)) == N.ADYPT_OK

    @staticmethod
    def last_error() -> str:
        return (N.lib.adypt_host_last_error() or b"").decode()

    # convenient attribute access with the reference's member names
    m_width = property(lambda s: s.c.width)
    m_height = property(lambda s: s.c.height)
    m_obj_filename = property(lambda s: s.c.obj_filename.decode())
    m_bvh_filename = property(lambda s: s.c.bvh_filename.decode())

    def pt_params(self, shift_seed: int = 0) -> N.PtParams:
        p = N.PtParams()
        p.stack_size, p.max_bounce, p.subpixel, p.tmp_lifetime = self.c.stack_size, self.c.max_bounce, self.c.subpixel, self.c.tmp_lifetime
        p.ray_tmin, p.clamp = self.c.ray_tmin, self.c.clamp
        p.sun[:] = list(self.c.sun)
        p.shift_seed = shift_seed
        return p

    def bvh_params(self) -> N.BvhParams:
        return N.BvhParams(self.c.bvh.max_spatial_depth, self.c.bvh.triangle_sah, self.c.bvh.node_sah)


class Scene:
    """Triangle[] + materials + decoded textures of an OBJ file."""

    def __init__(self) -> None:
        self._h = C.c_void_p()
        self.triangles = np.zeros(0, dtype=np.uint8)
        self.materials = np.zeros(0, dtype=np.uint8)
        self.textures: List[np.ndarray] = []
        self.warnings = ""

    def LoadFromFile(self, filename: str) -> bool:
        self._free()
        if N.lib.adypt_scene_load(filename.encode(), C.byref(self._h)) != N.ADYPT_OK:
            return False
        self._pull()
        return True

    @classmethod
    def FromArrays(cls, triangles: np.ndarray, materials: np.ndarray) -> "Scene":
        s = cls()
        t = np.ascontiguousarray(triangles).view(np.uint8).reshape(-1)
        m = np.ascontiguousarray(materials).view(np.uint8).reshape(-1)
        N.check_host(N.lib.adypt_scene_from_arrays(t.ctypes.data, len(t) // TRI_BYTES, m.ctypes.data, len(m) // MAT_BYTES, C.byref(s._h)))
        s._pull()
        return s

    def _pull(self) -> None:
        p = C.c_void_p()
        n = N.lib.adypt_scene_triangles(self._h, C.byref(p))
        self.triangles = _bytes_view(p.value, n * TRI_BYTES)
        n = N.lib.adypt_scene_materials(self._h, C.byref(p))
        self.materials = _bytes_view(p.value, n * MAT_BYTES)
        nt = N.lib.adypt_scene_textures(self._h, C.byref(p))
        self.textures = []
        if nt:
            arr = (N.Texture * nt).from_address(p.value)
            for t in arr:
                self.textures.append(_bytes_view(t.rgb, t.width * t.height * 3).reshape(t.height, t.width, 3))
        w = N.lib.adypt_scene_warnings(self._h)
        self.warnings = (w or b"").decode("utf-8", "replace")  # textures that could not be decoded (their materials render black)

    def GetTriangles(self) -> np.ndarray:
        return self.triangles

    def GetMaterials(self) -> np.ndarray:
        return self.materials

    def GetAABB(self) -> Tuple[np.ndarray, np.ndarray]:
        lo = np.zeros(3, dtype=np.float32)
        hi = np.zeros(3, dtype=np.float32)
        N.lib.adypt_scene_aabb(self._h, lo.ctypes.data, hi.ctypes.data)
        return lo, hi

    @property
    def n_tris(self) -> int:
        return len(self.triangles) // TRI_BYTES

    def _free(self) -> None:
        if self._h:
            N.lib.adypt_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:
        try:
            self._free()
        except Exception:
            pass


class WideBVH:
    """80-byte CWBVH8 nodes + reference->triangle indices (src/BVH/WideBVH.hpp:28-43)."""

    def __init__(self) -> None:
        self._h = C.c_void_p()
        self.nodes = np.zeros(0, dtype=np.uint8)
        self.tri_indices = np.zeros(0, dtype=np.int32)
        self.ref_boxes = np.zeros((0, 6), dtype=np.float32)  # of a tree with split triangles (BuildPLOC(split_budget=...)): lo xyz, hi xyz per reference
        self.build_info: Optional[N.BuildInfo] = None

    def _pull(self) -> None:
        p = C.c_void_p()
        n = N.lib.adypt_bvh_nodes(self._h, C.byref(p))
        self.nodes = _bytes_view(p.value, n * NODE_BYTES)
        n = N.lib.adypt_bvh_tri_indices(self._h, C.byref(p))
        self.tri_indices = _bytes_view(p.value, n * 4).view(np.int32)
        n = N.lib.adypt_bvh_ref_boxes(self._h, C.byref(p))
        self.ref_boxes = _bytes_view(p.value, n * 24).view(np.float32).reshape(-1, 6) if n else np.zeros((0, 6), dtype=np.float32)

    def LoadFromFile(self, filename: str, expected: N.BvhParams) -> bool:
        self._free()
        if N.lib.adypt_bvh_load(filename.encode(), C.byref(expected), C.byref(self._h)) != N.ADYPT_OK:
            return False
        self._pull()
        return True

    def SaveToFile(self, filename: str, cfg: N.BvhParams) -> bool:
        return N.lib.adypt_bvh_save(self._h, filename.encode(), C.byref(cfg)) == N.ADYPT_OK

    def Build(self, scene: Scene, cfg: N.BvhParams) -> None:
        """SBVHBuilder{cfg,&sbvh,scene}.Run(); WideBVHBuilder{cfg,&wbvh,sbvh}.Run() (src/Instance.cpp:24-26)."""
        self._free()
        info = N.BuildInfo()
        N.check_host(N.lib.adypt_bvh_build(scene._h, C.byref(cfg), C.byref(self._h), C.byref(info)))
        self.build_info = info
        self._pull()

    def BuildLinear(self, scene: Scene, cfg: N.BvhParams) -> None:
        """adypt_bvh_build_linear: the tree of a linear BVH (csrc/device/lbvh.hpp) — what RebuildBVH() builds on the GPU, byte for byte.  No spatial
        splits (cfg.max_spatial_depth is ignored): one reference per triangle."""
        self._free()
        info = N.BuildInfo()
        N.check_host(N.lib.adypt_bvh_build_linear(scene._h, C.byref(cfg), C.byref(self._h), C.byref(info)))
        self.build_info = info
        self._pull()

    def BuildPLOC(self, scene: Scene, cfg: N.BvhParams, radius: int = 8, split_budget: float = 0.0) -> None:
        """adypt_bvh_build_ploc: BuildLinear with the binary tree built bottom up by PLOC (csrc/device/ploc.hpp) — what RebuildBVH(method="ploc") builds
        on the GPU, byte for byte.  radius in [1, 32]: how far a cluster looks to either side in Morton order.  split_budget in [0, 1]
        (adypt_bvh_build_ploc_split, csrc/device/presplit.hpp): large triangles become several references with clipped boxes, at most
        split_budget * n more references than triangles; their boxes are ref_boxes.  0: no splits, the same bytes as ever."""
        self._free()
        info = N.BuildInfo()
        if split_budget == 0.0:
            N.check_host(N.lib.adypt_bvh_build_ploc(scene._h, C.byref(cfg), radius, C.byref(self._h), C.byref(info)))
        else:
            N.check_host(N.lib.adypt_bvh_build_ploc_split(scene._h, C.byref(cfg), radius, float(split_budget), C.byref(self._h), C.byref(info)))
        self.build_info = info
        self._pull()

    def Refit(self, scene: Scene) -> None:
        """adypt_bvh_refit: the boxes of the nodes recomputed, in place, for the triangles of `scene` as they are now (the same triangles, moved).
        The topology and GetTriIndices() stay; the Woop data of the pose is woop_matrices(scene.triangles, GetTriIndices())."""
        nodes = np.array(self.nodes, dtype=np.uint8)  # (all or nothing: self.nodes stays when the arrays are refused)
        t = np.ascontiguousarray(scene.triangles).view(np.uint8).reshape(-1)
        idx = np.ascontiguousarray(self.tri_indices, dtype=np.int32)
        N.check_host(N.lib.adypt_bvh_refit(nodes.ctypes.data, len(nodes) // NODE_BYTES, idx.ctypes.data, len(idx), t.ctypes.data, len(t) // TRI_BYTES))
        self.nodes = nodes

    def Cost(self, cfg: Optional[N.BvhParams] = None) -> dict:
        """adypt_bvh_cost: the SAH cost of the tree as the traversal sees it, from the quantised child boxes (csrc/device/tree_cost.hpp) — cost,
        and the two integer sums inner_q and leaf_q it is made of, and n_nodes.  What the tracers' GetTreeCost() measures on the GPU, to the same
        integers.  cfg None: triangleSAH 0.3, nodeSAH 1."""
        nodes = np.ascontiguousarray(self.nodes, dtype=np.uint8).reshape(-1)
        out = N.TreeCost()
        N.check_host(N.lib.adypt_bvh_cost(nodes.ctypes.data, len(nodes) // NODE_BYTES, None if cfg is None else C.byref(cfg), C.byref(out)))
        return out.as_dict()

    def GetNodes(self) -> np.ndarray:
        return self.nodes

    def GetTriIndices(self) -> np.ndarray:
        return self.tri_indices

    def _free(self) -> None:
        if self._h:
            N.lib.adypt_bvh_free(self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:
        try:
            self._free()
        except Exception:
            pass


TEST_HOOKS_MAGIC = 0x7465737468303031  # ADYPT_TEST_HOOKS_MAGIC (include/adypt_hip.h)


def enable_test_hooks() -> None:
    """TEST-ONLY (adypt_enable_test_hooks): makes the library honour ADYPT_MULTI_SHARED_DEVICE, ADYPT_COMM_TRANSPORT=host, ADYPT_AUDIT_SELFTEST and
    ADYPT_GATHER_STALL_TEST for the rest of this process.  tests/conftest.py, tools/comm_world.py and `bench.py --rehearsal` call it; nothing else does."""
    r = N.lib.adypt_enable_test_hooks(TEST_HOOKS_MAGIC)
    if r != N.ADYPT_OK:
        raise RuntimeError("adypt_enable_test_hooks refused")


def woop_matrices(triangles: np.ndarray, tri_indices: np.ndarray) -> np.ndarray:
    t = np.ascontiguousarray(triangles).view(np.uint8).reshape(-1)
    idx = np.ascontiguousarray(tri_indices, dtype=np.int32)
    out = np.empty((len(idx), 12), dtype=np.float32)
    N.lib.adypt_woop_matrices(t.ctypes.data, idx.ctypes.data, len(idx), out.ctypes.data)
    return out


def _pose_matrices(who: str, matrices) -> np.ndarray:
    """n x 12 float32 of matrices given as [n, 3, 4], [n, 12] or flat"""
    m = np.ascontiguousarray(matrices, dtype=np.float32)
    if m.size == 0 or m.size % 12:
        raise ValueError("%s: matrices are row-major 3x4, 12 floats each" % who)
    return m.reshape(-1, 12)


def _skin_arrays(who: str, joints, weights) -> Tuple[np.ndarray, np.ndarray]:
    """(uint16 [n, 12], float32 [n, 12]) of joints and weights given per triangle as [n, 3, 4], [n, 12] or flat"""
    j = np.asarray(joints)
    if j.size and (j.min() < 0 or j.max() > 65535):
        raise ValueError("%s: a joint index does not fit 16 bits" % who)
    j = np.ascontiguousarray(j, dtype=np.uint16).reshape(-1, 12)
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1, 12)
    if len(j) != len(w):
        raise ValueError("%s: joints and weights differ in length" % who)
    return j, w


def _morph_arrays(who: str, triangles, targets, deltas) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(int32 [n], int32 [n], float32 [n, 18]) of a morph layer's entries; deltas given as [n, 18] or [n, 2, 3, 3] (positions, normals) or flat"""
    t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1)
    k = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
    d = np.ascontiguousarray(deltas, dtype=np.float32)
    if d.size != 18 * len(t) or len(k) != len(t):
        raise ValueError("%s: an entry is a triangle, a target and 18 deltas" % who)
    return t, k, d.reshape(-1, 18)


def _morph_weights(morph_weights) -> np.ndarray:
    return np.ascontiguousarray(morph_weights, dtype=np.float32).reshape(-1)


def morph_diff(rest_triangles: np.ndarray, target_triangles: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """adypt_morph_diff: a dense target mesh as sparse morph entries.  (triangles int32 [k], deltas float32 [k, 18]) of the triangles whose positions
    or normals differ in any bit between two arrays of 100-byte triangles of equal count; deltas = target - rest in float32.  A weight of 1 gives
    rest + (target - rest): the target only up to one rounding."""
    a = np.ascontiguousarray(rest_triangles).view(np.uint8).reshape(-1)
    b = np.ascontiguousarray(target_triangles).view(np.uint8).reshape(-1)
    if len(a) != len(b) or len(a) % 100:
        raise ValueError("morph_diff: two arrays of 100-byte triangles of equal count")
    n = len(a) // 100
    k = N.lib.adypt_morph_diff(a.ctypes.data, b.ctypes.data, n, None, None)
    if k < 0:
        N.check_host(int(k))
    tri, d = np.empty(k, dtype=np.int32), np.empty((k, 18), dtype=np.float32)
    N.lib.adypt_morph_diff(a.ctypes.data, b.ctypes.data, n, tri.ctypes.data, d.ctypes.data)
    return tri, d


def pose_triangles(triangles: np.ndarray, matrices, parts=None, joints=None, weights=None, morph=None, morph_weights=None) -> np.ndarray:
    """adypt_pose_triangles, the host's side of Pose() (csrc/device/pose.hpp): the 100-byte triangles (uint8 [n * 100], or TRI_DT records) posed by
    row-major 3x4 matrices — by `parts` (one index per triangle) or by `joints` and `weights` (four per vertex: [n, 3, 4]).  Returns uint8 [n * 100];
    texture coordinates and material ids stay.  What BindParts / BindSkin / Pose refuse raises AdyptError here.
    morph: the (triangles, targets, deltas) triple of BindMorph(), applied under morph_weights (one per target) before the matrices
    (adypt_pose_triangles_morph): the host's side of Pose(..., morph_weights=...)."""
    if (morph is None) != (morph_weights is None):
        raise ValueError("pose_triangles: morph and morph_weights go together")
    t = np.ascontiguousarray(triangles).view(np.uint8).reshape(-1)
    m = _pose_matrices("pose_triangles", matrices)
    p = None if parts is None else np.ascontiguousarray(parts, dtype=np.int32).reshape(-1)
    j, w = (None, None) if joints is None or weights is None else _skin_arrays("pose_triangles", joints, weights)
    n = len(t) // 100
    for a in (p, j):
        if a is not None and len(a) != n:
            raise ValueError("pose_triangles: the binding is not of %d triangles" % n)
    out = np.empty_like(t)
    binding = (None if p is None else p.ctypes.data, None if j is None else j.ctypes.data, None if w is None else w.ctypes.data, m.ctypes.data, len(m))
    if morph is None:
        N.check_host(N.lib.adypt_pose_triangles(t.ctypes.data, n, *binding, out.ctypes.data))
        return out
    mt, mk, md = _morph_arrays("pose_triangles", *morph)
    mw = _morph_weights(morph_weights)
    N.check_host(N.lib.adypt_pose_triangles_morph(t.ctypes.data, n, *binding, mt.ctypes.data, mk.ctypes.data, md.ctypes.data, len(mt), mw.ctypes.data, len(mw), out.ctypes.data))
    return out


def _mesh_indices(who: str, indices, n_vertices: Optional[int]) -> Tuple[np.ndarray, int]:
    """(int32 [n, 3], n_vertices) of an index buffer given as [n, 3] or flat; n_vertices None: the largest index + 1"""
    i = np.ascontiguousarray(indices, dtype=np.int32)
    if i.size % 3:
        raise ValueError("%s: indices are three per triangle" % who)
    i = i.reshape(-1, 3)
    if n_vertices is None:
        n_vertices = int(i.max()) + 1 if i.size else 0
    return i, int(n_vertices)


def _vertex_array(who: str, a) -> np.ndarray:
    """float32 [n, 3] of one vector per vertex given as [n, 3] or flat"""
    v = np.ascontiguousarray(a, dtype=np.float32)
    if v.size % 3:
        raise ValueError("%s: three floats per vertex" % who)
    return v.reshape(-1, 3)


def mesh_normals(indices, positions, n_vertices: Optional[int] = None) -> np.ndarray:
    """adypt_mesh_normals, the host's side of PoseVertices() without normals (csrc/device/mesh.hpp): float32 [n_vertices, 3], a vertex's normal being
    the sum of its triangles' area-weighted face vectors in ascending corner order, normalised where its length is a positive finite number.  A
    vertex that no triangle names gets 0.  n_vertices None: len(positions)."""
    p = _vertex_array("mesh_normals", positions)
    i, nv = _mesh_indices("mesh_normals", indices, len(p) if n_vertices is None else n_vertices)
    if nv != len(p):
        raise ValueError("mesh_normals: %d positions for %d vertices" % (len(p), nv))
    out = np.empty_like(p)
    N.check_host(N.lib.adypt_mesh_normals(i.ctypes.data, len(i), nv, p.ctypes.data, out.ctypes.data))
    return out


def mesh_triangles(triangles: np.ndarray, indices, positions, normals=None) -> np.ndarray:
    """adypt_mesh_triangles, the host's side of BindMesh() + PoseVertices(): the 100-byte triangles (uint8 [n * 100], or TRI_DT records) with every
    corner's position and normal taken from its vertex — normals float32 [n_vertices, 3] used as given, or None: computed as mesh_normals() does.
    Returns uint8 [n * 100]; texture coordinates and material ids stay.  What BindMesh / PoseVertices refuse raises AdyptError here."""
    t = np.ascontiguousarray(triangles).view(np.uint8).reshape(-1)
    p = _vertex_array("mesh_triangles", positions)
    nrm = None if normals is None else _vertex_array("mesh_triangles", normals)
    i, nv = _mesh_indices("mesh_triangles", indices, len(p))
    if len(t) != 100 * len(i) or (nrm is not None and len(nrm) != len(p)):
        raise ValueError("mesh_triangles: 100-byte triangles, three indices each, and one position (and normal) per vertex")
    out = np.empty_like(t)
    N.check_host(N.lib.adypt_mesh_triangles(t.ctypes.data, len(i), i.ctypes.data, nv, p.ctypes.data, None if nrm is None else nrm.ctypes.data, out.ctypes.data))
    return out


def weld_triangles(triangles: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """adypt_weld_triangles: the index buffer of a triangle soup (anything that came through the OBJ loader).  (indices int32 [n, 3], positions
    float32 [n_vertices, 3], normals float32 [n_vertices, 3]); a vertex is a corner's position and normal compared as bits, numbered in order of
    first appearance, so a crease — one position, two normals — stays two vertices.  mesh_triangles(t, *weld_triangles(t)) has t's bytes."""
    t = np.ascontiguousarray(triangles).view(np.uint8).reshape(-1)
    if len(t) % 100:
        raise ValueError("weld_triangles: an array of 100-byte triangles")
    n = len(t) // 100
    nv = N.lib.adypt_weld_triangles(t.ctypes.data, n, None, None, None)
    if nv < 0:
        N.check_host(int(nv))
    idx, p, nrm = np.empty((n, 3), dtype=np.int32), np.empty((nv, 3), dtype=np.float32), np.empty((nv, 3), dtype=np.float32)
    N.lib.adypt_weld_triangles(t.ctypes.data, n, idx.ctypes.data, p.ctypes.data, nrm.ctypes.data)
    return idx, p, nrm


# struct RootCard (csrc/device/root_card.hpp), 264 bytes; q[child] = float(qlo x, qhi x, qlo y, qhi y, qlo z, qhi z)
ROOT_CARD_DT = np.dtype([("q", "<f4", (8, 6)), ("scale", "<f4", 3), ("origin", "<f4", 3), ("child_base", "<u4"), ("tri_base", "<u4"), ("imask", "<u4"),
                         ("inner_only", "<u4"), ("enabled", "<u4"), ("pad", "<u4"), ("is_inner", "u1", 8), ("bit_index", "u1", 8), ("child_bits", "u1", 8)])


def _materials_array(who: str, materials) -> np.ndarray:
    """The material table as bytes: a whole number of 64-byte GPUMaterial records (none is allowed)."""
    m = np.ascontiguousarray(materials).view(np.uint8).reshape(-1)
    if len(m) % MAT_BYTES:
        raise ValueError("%s: the materials are not a whole number of %d-byte records" % (who, MAT_BYTES))
    return m


def _texture_table(who: str, textures) -> tuple:
    """(adypt_texture array or None, count, what it points into) of a sequence of uint8 [h, w, 3] images; sizes and pointers are the library's to refuse."""
    tex = [np.ascontiguousarray(t, dtype=np.uint8) for t in textures]
    for t in tex:
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("%s: a texture is uint8 [height, width, 3]" % who)
    arr = (N.Texture * max(1, len(tex)))()
    for i, t in enumerate(tex):
        arr[i].width, arr[i].height, arr[i].rgb = t.shape[1], t.shape[0], (t.ctypes.data if t.size else None)
    return (C.addressof(arr) if tex else None), len(tex), [arr] + tex


def pack_appearance(materials, textures=()) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The device's material table and texture arena of a scene, made on the host (adypt_pack_appearance; the definition: csrc/device/appearance.hpp):
    (records uint32 [n_mats, 20], texels uint32 [words], descriptors int32 [n_textures, 4] = (offset, w, h, 0)) — what ReadMaterialRecords() and
    ReadTexels() give after Initialize or SetMaterials with the same arrays, byte for byte."""
    m = _materials_array("pack_appearance", materials)
    tex, n_tex, keep = _texture_table("pack_appearance", textures)
    args = (m.ctypes.data if len(m) else None, len(m) // MAT_BYTES, tex, n_tex)
    words = N.lib.adypt_pack_appearance(*args, None, None, None)
    if words < 0:
        raise N.AdyptError(int(words), "adypt_pack_appearance: a texture without pixels, or 2^31 texels and more")
    rec, texels, desc = np.zeros((len(m) // MAT_BYTES, 20), np.uint32), np.zeros(int(words), np.uint32), np.zeros((n_tex, 4), np.int32)
    r = N.lib.adypt_pack_appearance(*args, rec.ctypes.data, texels.ctypes.data, desc.ctypes.data)
    assert r == words and keep
    return rec, texels, desc


def decode_root_card(node: np.ndarray, allow: bool = True) -> np.ndarray:
    """adypt_decode_root_card: one 80-byte node as the ROOT_CARD_DT record k_path's shading round tests new rays against."""
    n = np.ascontiguousarray(node).view(np.uint8).reshape(-1)
    if len(n) != NODE_BYTES:
        raise ValueError("decode_root_card: a node is %d bytes" % NODE_BYTES)
    card = np.zeros(1, dtype=ROOT_CARD_DT)
    N.lib.adypt_decode_root_card(n.ctypes.data, 1 if allow else 0, card.ctypes.data)
    return card[0]


def sobol_points(dim: int, first: int, n: int) -> np.ndarray:
    out = np.empty((n, dim), dtype=np.float32)
    N.check_host(N.lib.adypt_sobol_points(dim, first, n, out.ctypes.data))
    return out


def shift_bytes(seed: int, width: int, height: int) -> np.ndarray:
    out = np.empty((height, width, 2), dtype=np.uint8)
    N.lib.adypt_shift_bytes(seed, width, height, out.ctypes.data)
    return out


def save_exr(path: str, rgb: np.ndarray, save_as_fp16: bool = False) -> None:
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[:2]
    N.check_host(N.lib.adypt_save_exr(path.encode(), rgb.ctypes.data, w, h, 1 if save_as_fp16 else 0))


def save_png(path: str, rgba8: np.ndarray) -> None:
    rgba8 = np.ascontiguousarray(rgba8, dtype=np.uint8)
    h, w = rgba8.shape[:2]
    assert rgba8.shape == (h, w, 4)
    N.check_host(N.lib.adypt_save_png(path.encode(), rgba8.ctypes.data, w, h))


def load_image_rgb8(path: str) -> np.ndarray:
    """stbi_load(path, &w, &h, &c, 3) of OglScene::load_texture: H x W x 3 uint8, row 0 = top."""
    p, w, h = C.c_void_p(), C.c_int32(), C.c_int32()
    N.check_host(N.lib.adypt_load_image_rgb8(path.encode(), C.byref(p), C.byref(w), C.byref(h)))
    try:
        return np.array(_bytes_view(p.value, w.value * h.value * 3).reshape(h.value, w.value, 3))
    finally:
        N.lib.adypt_free(p)


def load_exr(path: str) -> np.ndarray:
    p = C.c_void_p()
    w = C.c_int()
    h = C.c_int()
    N.check_host(N.lib.adypt_load_exr(path.encode(), C.byref(p), C.byref(w), C.byref(h)))
    out = np.frombuffer((C.c_float * (w.value * h.value * 3)).from_address(p.value), dtype=np.float32).copy().reshape(h.value, w.value, 3)
    N.lib.adypt_free(p)
    return out


class Camera:
    """Camera::Initialize / GetView / GetProjection / Control (src/Tracer/Camera.hpp:14-37)."""

    def Initialize(self, cfg: InstanceConfig, width: int, height: int) -> None:
        self.cfg, self.width, self.height = cfg, width, height

    def matrices(self) -> Tuple[np.ndarray, np.ndarray]:
        ip = np.empty(16, dtype=np.float32)
        iv = np.empty(16, dtype=np.float32)
        c = self.cfg.c
        N.lib.adypt_camera_matrices(c.fov, c.yaw, c.pitch, self.width, self.height, ip.ctypes.data, iv.ctypes.data)
        return ip, iv

    @property
    def position(self) -> np.ndarray:
        return np.array(list(self.cfg.c.position), dtype=np.float32)

    KEY_W, KEY_A, KEY_S, KEY_D, KEY_SPACE, KEY_LEFT_SHIFT = 1, 2, 4, 8, 16, 32

    def Control(self, keys: int = 0, mouse_dx: float = 0.0, mouse_dy: float = 0.0, frame_seconds: float = 0.0) -> None:
        """Camera::Control (src/Tracer/Camera.cpp:25-59) with the key / mouse state passed in instead of read from GLFW."""
        N.lib.adypt_camera_control(C.byref(self.cfg.c), keys, mouse_dx, mouse_dy, frame_seconds)


def camera_matrices(fov: float, yaw: float, pitch: float, width: int, height: int) -> Tuple[np.ndarray, np.ndarray]:
    ip = np.empty(16, dtype=np.float32)
    iv = np.empty(16, dtype=np.float32)
    N.lib.adypt_camera_matrices(fov, yaw, pitch, width, height, ip.ctypes.data, iv.ctypes.data)
    return ip, iv


def device_free_bytes(device: int) -> Optional[int]:
    """Free memory of HIP device `device` (hipMemGetInfo through the runtime libadypt_hip.so is linked against), None when the runtime does not answer.
    Measurement scripts only (bench.py's self-check asks before it creates a second context of a large scene); the library itself never asks."""
    try:
        hip = C.CDLL("libamdhip64.so")
        free, total = C.c_size_t(0), C.c_size_t(0)
        if hip.hipSetDevice(C.c_int(device)) != 0 or hip.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
            return None
        return int(free.value)
    except OSError:
        return None


class HipScene:
    """OglScene: the flat arrays the kernels consume.  Initialize(scene, bvh) only records host arrays; the upload
    to HBM happens in HipPathTracer.Initialize (adypt_create) because the C-ABI creates scene + images together."""

    def Initialize(self, scene: Scene, bvh: Optional[WideBVH] = None, woop: Optional[np.ndarray] = None) -> None:
        """bvh None: the tracer builds the first tree on the GPU from the triangles (adypt_create_from_triangles)."""
        if bvh is None and woop is not None:
            raise ValueError("HipScene.Initialize: Woop data need the tree they were computed for")
        self.scene, self.bvh = scene, bvh
        self.woop = None if woop is None else np.ascontiguousarray(woop, dtype=np.float32)

    def GetTextures(self) -> Sequence[np.ndarray]:
        return self.scene.textures


class ViewerTypes:
    kDiffuse, kSpecular, kEmissive, kPTRadiance, kNormal, kPosition = range(6)


def _scene_desc(scene: HipScene, width: int, height: int) -> Tuple[N.SceneDesc, list]:
    """adypt_scene_desc of `scene` for device 0 and the whole image, and the arrays it points into (to be kept alive while it is in use)."""
    s, b = scene.scene, scene.bvh
    tex_arr = (N.Texture * max(1, len(s.textures)))()
    keep = [s.triangles, s.materials, scene.woop, tex_arr] + list(s.textures) + ([] if b is None else [b.nodes, b.tri_indices])
    for i, t in enumerate(s.textures):
        tex_arr[i].width, tex_arr[i].height, tex_arr[i].rgb = t.shape[1], t.shape[0], t.ctypes.data
    d = N.SceneDesc()
    if b is not None:  # (else: no tree, every field of it null)
        d.nodes, d.n_nodes = b.nodes.ctypes.data, len(b.nodes) // NODE_BYTES
        d.tri_indices, d.n_refs = b.tri_indices.ctypes.data, len(b.tri_indices)
    d.woop = None if scene.woop is None else scene.woop.ctypes.data
    d.triangles, d.n_tris = s.triangles.ctypes.data, len(s.triangles) // TRI_BYTES
    d.materials, d.n_mats = (s.materials.ctypes.data if len(s.materials) else None), len(s.materials) // MAT_BYTES
    d.textures, d.n_textures = (C.addressof(tex_arr) if s.textures else None), len(s.textures)
    d.width, d.height, d.device, d.tile_rank, d.tile_nranks = width, height, 0, 0, 1
    return d, keep


def _build_args(who: str, cfg: Optional[N.BvhParams], method: str, radius: int, split_budget: float, split_needs_ploc: bool = True) -> tuple:
    """(params, method, radius, split_budget) as every entry that builds a tree takes them (csrc/device/build_request.hpp); what only Python can get wrong is
    refused here, everything else by the library — with split_needs_ploc False a split_budget with "linear" too."""
    if method not in ("linear", "ploc"):
        raise ValueError("%s: method must be 'linear' or 'ploc', not %r" % (who, method))
    if split_needs_ploc and split_budget != 0.0 and method != "ploc":
        raise ValueError("%s: split_budget needs method 'ploc'" % who)
    return (None if cfg is None else C.byref(cfg), 1 if method == "ploc" else 0, int(radius), float(split_budget))


def _set_triangles_args(who: str, triangles: Optional[np.ndarray], cfg: Optional[N.BvhParams], method: str, radius: int, split_budget: float) -> tuple:
    """(triangles, n_tris, params, method, radius, split_budget) of adypt_set_triangles / adypt_create_from_triangles (the latter takes the last four)"""
    build = _build_args(who, cfg, method, radius, split_budget, split_needs_ploc=False)
    if triangles is None:  # (the library's refusal to give)
        return (None, 1) + build
    t = np.ascontiguousarray(triangles).view(np.uint8).reshape(-1)
    if len(t) % TRI_BYTES:
        raise ValueError("%s: the triangles are not a whole number of %d-byte records" % (who, TRI_BYTES))
    return (t.ctypes.data, len(t) // TRI_BYTES) + build


def _read_block_noise(ctx) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """adypt_read_block_noise on one context: the size first, then the blocks."""
    n = N.lib.adypt_read_block_noise(ctx, None, None, None, 0)
    if n < 0:
        N.check(int(n), ctx)
    idx, s, cnt = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.uint32)
    if n:
        r = N.lib.adypt_read_block_noise(ctx, idx.ctypes.data, s.ctypes.data, cnt.ctypes.data, n)
        if r < 0:
            N.check(int(r), ctx)
    return idx, s, cnt


def _read_block_spp(ctx) -> Tuple[np.ndarray, np.ndarray]:
    """adypt_read_block_spp on one context: the size first, then the blocks."""
    n = N.lib.adypt_read_block_spp(ctx, None, None, 0)
    if n < 0:
        N.check(int(n), ctx)
    idx, spp = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    if n:
        r = N.lib.adypt_read_block_spp(ctx, idx.ctypes.data, spp.ctypes.data, n)
        if r < 0:
            N.check(int(r), ctx)
    return idx, spp


def _blocks_by_index(parts) -> Tuple[np.ndarray, ...]:
    """The contexts' per-block arrays (block index first) as one set, ascending block index: every block has one owner, and one context's list is
    ascending already."""
    cols = [np.concatenate(col) for col in zip(*parts)]
    order = np.argsort(cols[0], kind="stable")
    return tuple(col[order] for col in cols)


class _Tracer:
    """What HipPathTracer and MultiPathTracer both offer, written once over three things the class gives: the handle `_h`, the symbol family
    `_family` ("adypt_" or "adypt_multi_": `_call("trace_spp", n)` is adypt_trace_spp or adypt_multi_trace_spp on the handle) and its own error
    reader `_check(code)`.  What the C-ABI offers per context only goes through `_contexts()`."""
    _family = ""
    _destroy = ""

    def __init__(self) -> None:
        self._h = C.c_void_p()
        self.m_viewer_type = ViewerTypes.kDiffuse

    def _fn(self, name: str):
        return getattr(N.lib, self._family + name)

    def _call(self, name: str, *args) -> None:
        self._check(self._fn(name)(self._h, *args))

    def SetConfig(self, config: N.PtParams) -> None:
        self._call("set_params", C.byref(config))

    def SetCamera(self, inv_projection: np.ndarray, inv_view: np.ndarray, position) -> None:
        ip = np.ascontiguousarray(inv_projection, dtype=np.float32).reshape(16)
        iv = np.ascontiguousarray(inv_view, dtype=np.float32).reshape(16)
        pos = np.ascontiguousarray(position, dtype=np.float32).reshape(3)
        self._call("set_camera", pos.ctypes.data, ip.ctypes.data, iv.ctypes.data)

    def Trace(self, enable_pt: bool, n_spp: int = 1) -> None:
        """Trace(true): n_spp more frames; Trace(false): one primary-ray viewer frame of m_viewer_type."""
        if enable_pt:
            self.m_viewer_type = ViewerTypes.kPTRadiance
            self._call("trace_spp", n_spp)
        else:
            if self.m_viewer_type == ViewerTypes.kPTRadiance:
                self.m_viewer_type = ViewerTypes.kDiffuse
            self._call("trace_primary", self.m_viewer_type)

    def SetSunVisibility(self, enabled: bool, direction=None) -> None:
        """The occlusion query the reference has commented out (pathtracer.glsl:132); off = the reference as it runs."""
        d = None if direction is None else np.ascontiguousarray(direction, dtype=np.float32).reshape(3)
        self._call("set_sun_visibility", 1 if enabled else 0, None if d is None else d.ctypes.data)

    def SetLookahead(self, enabled: bool) -> None:
        """One Trace(true) per call (Instance::Update) at batched throughput: see adypt_set_lookahead."""
        self._call("set_lookahead", 1 if enabled else 0)

    def Reset(self) -> None:
        self._call("reset")

    def GetSPP(self) -> int:
        return self._fn("get_spp")(self._h)

    def CommRanks(self) -> int:
        """Ranks of the communicator as RCCL reports them (ncclCommCount); 0 = none (one device, the shared-device test hook)."""
        return self._fn("comm_ranks")(self._h)

    def GetStats(self) -> dict:
        """Several devices: counts summed over them, kernel times of the slowest one (they run concurrently)."""
        st = N.Stats()
        self._call("get_stats", C.byref(st))
        return st.as_dict()

    # ---- per context ----
    def GetFramesInFlight(self) -> int:
        return N.lib.adypt_get_frames_in_flight(self._contexts()[0])

    def GetFusedBounces(self) -> bool:
        """Whether the last batch of frames ran its bounces in one launch."""
        return N.lib.adypt_get_fused_bounces(self._contexts()[0]) == 1

    def ResetStats(self) -> None:
        for c in self._contexts():
            N.check(N.lib.adypt_reset_stats(c), c)

    def DeviceSynchronize(self) -> None:
        for c in self._contexts():
            N.check(N.lib.adypt_device_synchronize(c), c)

    def GetShaderClockGHz(self) -> float:
        """Clock the chip held under the traversal launches since ResetStats (s_memtime / s_memrealtime of workgroup 0); 0.0 if none ran."""
        out = (C.c_uint64 * 2)()
        c = self._contexts()[0]
        N.check(N.lib.adypt_get_shader_clock(c, out), c)
        return float(out[0]) / float(out[1]) * 0.1 if out[1] else 0.0

    # ---- noise statistics (adypt_set_noise_stats, include/adypt_hip.h); several devices: of the whole image, the devices' blocks merged on the host ----
    def SetNoiseStats(self, enabled: bool) -> None:
        """Per-pixel luminance moments next to the running mean; enable at 0 spp.  The image never changes."""
        self._call("set_noise_stats", 1 if enabled else 0)

    def GetNoiseStats(self) -> bool:
        return N.lib.adypt_get_noise_stats(self._contexts()[0]) == 1

    def GetNoise(self) -> dict:
        """mean_noise, worst_block, worst_index, spp, pixels of the blocks this tracer owns (needs >= 2 spp)."""
        out = N.Noise()
        self._call("get_noise", C.byref(out))
        return out.as_dict()

    def ReadNoise(self) -> np.ndarray:
        """H x W float32: the relative standard error of every pixel's mean luminance."""
        e = np.zeros((self.height, self.width), dtype=np.float32)
        self._call("read_noise", e.ctypes.data)
        return e

    def ReadNoiseMoments(self) -> np.ndarray:
        """H x W x 2 float32: (mean, m2) of every pixel's luminance.  Every context writes the pixels of its own tiles."""
        m = np.zeros((self.height, self.width, 2), dtype=np.float32)
        for c in self._contexts():
            N.check(N.lib.adypt_read_noise_moments(c, m.ctypes.data), c)
        return m

    def TraceUntil(self, target: float, min_spp: int = 16, max_spp: int = 1024, check_every: int = 16) -> dict:
        """Trace(true) in steps of check_every until worst_block <= target (and spp >= min_spp) or spp >= max_spp; the last GetNoise()."""
        self.m_viewer_type = ViewerTypes.kPTRadiance
        out = N.Noise()
        self._call("trace_until", float(target), min_spp, max_spp, check_every, C.byref(out))
        return out.as_dict()

    # ---- adaptive sampling (adypt_trace_adaptive, include/adypt_hip.h): blocks at the noise target stop being traced ----
    def TraceAdaptive(self, target: float, min_spp: int = 16, max_spp: int = 1024, check_every: int = 16) -> dict:
        """Trace(true) in steps of check_every; from min_spp on every 32x32 block whose mean noise is <= target is frozen at its sample count.  Ends
        when no block is active or at max_spp.  The noise numbers of all blocks (each at its own count), blocks, blocks_frozen, pixel_samples."""
        self.m_viewer_type = ViewerTypes.kPTRadiance
        out = N.Adaptive()
        self._call("trace_adaptive", float(target), min_spp, max_spp, check_every, C.byref(out))
        return out.as_dict()

    def ReadBlockSPP(self) -> Tuple[np.ndarray, np.ndarray]:
        """(block index int32, sample count int32) of every 32x32 block this tracer owns, ascending block index."""
        return _blocks_by_index([_read_block_spp(c) for c in self._contexts()])

    def ReadBlockNoise(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(block index int32, sum float64, count uint32) of every 32x32 block this tracer owns, ascending block index (needs >= 2 spp)."""
        return _blocks_by_index([_read_block_noise(c) for c in self._contexts()])

    def ReadSPP(self) -> np.ndarray:
        """H x W int32: the sample count of every pixel, built from the blocks (0 where no context of this tracer owns the block)."""
        out = np.zeros((self.height, self.width), dtype=np.int32)
        nbx = (self.width + 31) // 32
        for b, n in zip(*self.ReadBlockSPP()):
            by, bx = divmod(int(b), nbx)
            out[by * 32:(by + 1) * 32, bx * 32:(bx + 1) * 32] = n
        return out

    # ---- history-aware sampling (adypt_plan_by_history, include/adypt_hip.h; the definition: csrc/device/history_reach.hpp) ----
    def _by_history(self, name, target, min_spp, max_spp, step, tolerance_permille, history_cap, follow_motion, moments) -> dict:
        prm = N.HistoryPlanParams(target, min_spp, max_spp, step, tolerance_permille, history_cap, 1 if follow_motion else 0, 1 if moments else 0)
        out = N.HistoryPlan()
        self._call(name, C.byref(prm), C.byref(out))
        return out.as_dict()

    def PlanByHistory(self, target: int, min_spp: int = 2, max_spp: int = 64, step: int = 4, tolerance_permille: int = 31,
                      history_cap: float = 64.0, follow_motion: bool = False, moments: bool = False) -> dict:
        """Before the first sample of a pose (GetSPP() == 0, nothing frozen, the camera set, the noise statistics on): captures the primary-hit guides,
        works out how many samples of history Denoise(temporal=True[, follow_motion][, moments]) WILL find at every pixel (ReadHistoryReach) and gives
        every 32x32 block the smallest sample count of min_spp, min_spp + step, ..., max_spp that leaves at most tolerance_permille / 1000 of its hit
        pixels below `target` samples of history and own samples together (ReadSamplePlan).  Traces nothing, freezes nothing, and leaves the history
        and every later Denoise() as they were.  Not covered: rectify (the plan may overestimate the history there) and follow_specular.
        blocks, want_min, want_max, spp, pixels, pixels_with_history, pixel_samples, mean_reach, capture_ms, reach_ms, device_bytes."""
        return self._by_history("plan_by_history", target, min_spp, max_spp, step, tolerance_permille, history_cap, follow_motion, moments)

    def TraceByHistory(self, target: int, min_spp: int = 2, max_spp: int = 64, step: int = 4, tolerance_permille: int = 31,
                       history_cap: float = 64.0, follow_motion: bool = False, moments: bool = False) -> dict:
        """PlanByHistory, then the tracing it asks for: the distinct sample counts in ascending order, the blocks of each frozen at it (a frozen block
        holds the bits of the uniform image at its count), the blocks of the largest left active.  ReadBlockSPP() is ReadSamplePlan() afterwards."""
        self.m_viewer_type = ViewerTypes.kPTRadiance
        return self._by_history("trace_by_history", target, min_spp, max_spp, step, tolerance_permille, history_cap, follow_motion, moments)

    def ReadHistoryReach(self) -> np.ndarray:
        """H x W float32: the samples of history every pixel will find, of the last plan (0: a miss, or no history)."""
        r = np.zeros((self.height, self.width), dtype=np.float32)
        self._call("read_history_reach", r.ctypes.data)
        return r

    def _read_plan(self, name: str, per_block: int, dtype) -> Tuple[np.ndarray, np.ndarray]:
        n = self._fn(name)(self._h, None, None, 0)
        if n < 0:
            self._check(int(n))
        idx, v = np.zeros(n, dtype=np.int32), np.zeros((n, per_block) if per_block > 1 else n, dtype=dtype)
        if n:
            r = self._fn(name)(self._h, idx.ctypes.data, v.ctypes.data, n)
            if r < 0:
                self._check(int(r))
        return idx, v

    def ReadSamplePlan(self) -> Tuple[np.ndarray, np.ndarray]:
        """(block index int32, planned sample count int32) of every 32x32 block of the last plan, ascending block index."""
        return self._read_plan("read_sample_plan", 1, np.int32)

    def ReadHistoryBins(self) -> Tuple[np.ndarray, np.ndarray]:
        """(block index int32, bins uint32 (blocks, 65)) of the last plan: bins[i, k] = the hit pixels of block i inside the image whose reach has
        floor k (k == 64: a reach of 64 or more)."""
        return self._read_plan("read_history_bins", 65, np.uint32)

    # ---- denoising (adypt_denoise, include/adypt_hip.h; the definition: csrc/device/denoise.hpp); several devices: of the whole image ----
    def Denoise(self, levels: int = 5, sigma_l: float = 4.0, sigma_z: float = 0.1, temporal: bool = False, history_cap: float = 64.0,
                commit: bool = True, follow_motion: bool = False, rectify: bool = False, rectify_radius: int = 3, rectify_gamma: float = 1.0,
                specular_bounces: int = 0, moments: bool = False, follow_specular: int = 0) -> np.ndarray:
        """H x W x 3 float32: the accumulated image through the variance- and primary-hit-guided a-trous filter.  Needs the noise statistics on and
        >= 2 spp in every block (moments: 1); the image, the statistics and the tracing state are left as they are.
        temporal (adypt_denoise_temporal; the definition: csrc/device/temporal.hpp): before the filter, what the last committing call left is
        reprojected through the primary hit and counted as up to history_cap further samples where the surface is still the same; commit: this
        call's state replaces that history (once per pose: after tracing, before the camera or the scene changes).  Give every pose a shift_seed of
        its own (SetConfig): after a reset an unchanged camera with an unchanged seed repeats the same samples.
        follow_motion (adypt_denoise_temporal_motion; needs temporal): a committing call also keeps every triangle's positions and normals, and a
        later call merges a pixel on a triangle that UpdateTriangles() or Pose() has moved since through the point its hit had then — the moved
        figure keeps its history.  Give it to every call of an animation; SetTriangles() and a committing call without it start the figure again.
        rectify (adypt_denoise_temporal_rectified; needs temporal; the definition: csrc/device/rectify.hpp): the history is held against the mean of
        the (2 rectify_radius + 1)^2 window of this call's own image on the pixel's surface and clamped to within rectify_gamma standard deviations
        of it, and loses length by as much as it disagrees — for light that changed on a surface that stands still (a shadow that wandered, another
        sun).  rectify_radius in [1, 3], rectify_gamma a finite number >= 0.  Combines with follow_motion.
        specular_bounces (adypt_denoise_specular; the definition: csrc/device/guide_chain.hpp): 0 is the call above to the bit; K in [1, 8] guides a
        pixel whose primary hit is a perfect mirror or glass by the first surface its chain of up to K reflections / transmissions ends on, and
        keeps pixels of different chain classes from pooling.  Not together with temporal: its temporal form is follow_specular.
        moments (adypt_denoise_temporal_moments; needs temporal; the definition: csrc/device/moments.hpp): the call runs from 1 spp in every block.
        The history carries the second moment of the demodulated luminance instead of a variance, and the variance the filter sees is made after the
        merge: from the moments where the merged history is at least 4 samples long, from a 7 x 7 window on the pixel's surface where it is
        shorter.  A moments call and a plain temporal call do not find each other's history.  Combines with follow_motion; not with rectify (the
        clamp would leave the moment inconsistent with the colour) and not with specular_bounces.
        follow_specular (adypt_denoise_temporal_specular; needs temporal; the definitions: guide_chain.hpp, temporal.hpp): 0 is off; K in [1, 8] is the
        temporal call with the guides of specular_bounces=K, and a pixel whose chain ended on a surface finds its history through its virtual point —
        the camera ray unfolded to the chain's full length, of a planar mirror the mirror image of what it shows — with every tap held against the
        followed guides and the pixel's class.  Such a call finds only a history a call with the same K left, and the other temporal calls none in
        its.  history_cap and commit as above; not with specular_bounces, follow_motion, rectify or moments."""
        if follow_specular != 0:
            if not temporal:
                raise ValueError("Denoise: follow_specular needs temporal=True")
            if not 1 <= follow_specular <= 8:
                raise ValueError("Denoise: follow_specular must be 0 or in [1, 8]")
            if specular_bounces or follow_motion or rectify or moments:
                raise ValueError("Denoise: follow_specular does not combine with specular_bounces, follow_motion, rectify or moments")
        if moments and not temporal:
            raise ValueError("Denoise: moments=True needs temporal=True")
        if moments and rectify:
            raise ValueError("Denoise: moments=True does not combine with rectify=True (the clamp would leave the second moment inconsistent with the colour)")
        if moments and specular_bounces:
            raise ValueError("Denoise: moments=True does not combine with specular_bounces")
        if follow_motion and not temporal:
            raise ValueError("Denoise: follow_motion=True needs temporal=True")
        if rectify and not temporal:
            raise ValueError("Denoise: rectify=True needs temporal=True")
        if specular_bounces != 0 and not 1 <= specular_bounces <= 8:
            raise ValueError("Denoise: specular_bounces must be 0 or in [1, 8]")
        if specular_bounces and temporal:
            raise ValueError("Denoise: specular_bounces has no temporal form (the merge reprojects the position guide through the camera)")
        prm = N.DenoiseParams(levels, sigma_l, sigma_z)
        if follow_specular:
            tp, sp = N.TemporalParams(history_cap, 1 if commit else 0), N.SpecularParams(follow_specular)
            self._call("denoise_temporal_specular", C.byref(prm), C.byref(tp), C.byref(sp))
        elif specular_bounces:
            sp = N.SpecularParams(specular_bounces)
            self._call("denoise_specular", C.byref(prm), C.byref(sp))
        elif moments:
            tp = N.TemporalParams(history_cap, 1 if commit else 0)
            self._call("denoise_temporal_moments", C.byref(prm), C.byref(tp), 1 if follow_motion else 0)
        elif temporal and rectify:
            tp, rp = N.TemporalParams(history_cap, 1 if commit else 0), N.RectifyParams(rectify_radius, rectify_gamma)
            self._call("denoise_temporal_rectified", C.byref(prm), C.byref(tp), C.byref(rp), 1 if follow_motion else 0)
        elif temporal:
            tp = N.TemporalParams(history_cap, 1 if commit else 0)
            self._call("denoise_temporal_motion" if follow_motion else "denoise_temporal", C.byref(prm), C.byref(tp))
        else:
            self._call("denoise", C.byref(prm))
        rgb = np.zeros((self.height, self.width, 3), dtype=np.float32)
        self._call("read_denoised", rgb.ctypes.data)
        return rgb

    def ResetDenoiseHistory(self) -> None:
        """Drops the history of Denoise(temporal=True): the next such call is the plain filter."""
        self._call("denoise_history_reset")

    def ReadDenoiseHistory(self) -> np.ndarray:
        """H x W float32: the effective sample count of every pixel after the last Denoise(temporal=True) (the block's own where it took no history)."""
        n = np.zeros((self.height, self.width), dtype=np.float32)
        self._call("read_denoise_history", n.ctypes.data)
        return n

    def ReadDenoiseMotion(self) -> dict:
        """Of the last Denoise(temporal=True, follow_motion=True): previous_position (H x W x 3 float32: where every pixel's hit point was when the
        history was committed; the current position where nothing moved) and moved (H x W bool: the hit triangle has moved since)."""
        p = np.zeros((self.height, self.width, 3), dtype=np.float32)
        moved = np.zeros((self.height, self.width), dtype=np.uint8)
        self._call("read_denoise_motion", p.ctypes.data, moved.ctypes.data)
        return {"previous_position": p, "moved": moved.astype(bool)}

    def GetDenoiseMotion(self) -> dict:
        """have_snapshot (0 / 1), snapshot_ms, n_tris and device_bytes of what follow_motion keeps on the (first) device."""
        out = N.DenoiseMotion()
        self._call("get_denoise_motion", C.byref(out))
        return out.as_dict()

    def ReadDenoiseRectify(self) -> np.ndarray:
        """H x W float32: the share of its length every pixel's history kept in the last Denoise(temporal=True, rectify=True) (1 where the pixel found
        no history, or its window had too few taps to say anything)."""
        kept = np.zeros((self.height, self.width), dtype=np.float32)
        self._call("read_denoise_rectify", kept.ctypes.data)
        return kept

    def GetDenoiseRectify(self) -> dict:
        """have (0 / 1), radius, gamma and window_ms (the window kernel's HIP-event milliseconds) of the last rectified call, and device_bytes of what
        rectify keeps on the (first) device."""
        out = N.DenoiseRectify()
        self._call("get_denoise_rectify", C.byref(out))
        return out.as_dict()

    def ReadDenoiseVariance(self) -> np.ndarray:
        """H x W float32: the variance the first level saw at every pixel in the last Denoise(temporal=True, moments=True)."""
        v = np.zeros((self.height, self.width), dtype=np.float32)
        self._call("read_denoise_variance", v.ctypes.data)
        return v

    def GetDenoiseMoments(self) -> dict:
        """have (0 / 1), variance_ms (the variance kernel's HIP-event milliseconds) and pixels_spatial (the pixels that took the window estimate) of the
        last moments call, and device_bytes of what moments keeps on the (first) device: the variance read-out and the count."""
        out = N.DenoiseMoments()
        self._call("get_denoise_moments", C.byref(out))
        return out.as_dict()

    def GetDenoiseMergeMs(self) -> float:
        """HIP-event milliseconds of the merge kernel of the last Denoise(temporal=True) (with follow_motion: of the gather kernel and the merge kernel;
        with rectify: of the window kernel too; with moments: of the variance kernel too)."""
        ms = C.c_float(0.0)
        self._call("get_denoise_merge_ms", C.byref(ms))
        return float(ms.value)

    def ReadDenoiseGuides(self, specular_bounces: int = 0) -> dict:
        """The feature images of the pixel-centre camera ray under the current camera: albedo, normal, position (H x W x 3 float32) and hit (H x W bool).
        specular_bounces K in [1, 8]: the guides Denoise(specular_bounces=K) filters with, and chain (H x W int8): every pixel's class code — 0 a
        primary miss, 1 a primary hit that is followed nowhere, 1 + L a chain that ended on a surface after L bounces, -(L + 1) one that left the scene."""
        a, n, p = (np.zeros((self.height, self.width, 3), dtype=np.float32) for _ in range(3))
        hit = np.zeros((self.height, self.width), dtype=np.uint8)
        if specular_bounces == 0:
            self._call("read_denoise_guides", a.ctypes.data, n.ctypes.data, p.ctypes.data, hit.ctypes.data)
            return {"albedo": a, "normal": n, "position": p, "hit": hit.astype(bool)}
        if not 1 <= specular_bounces <= 8:
            raise ValueError("ReadDenoiseGuides: specular_bounces must be 0 or in [1, 8]")
        chain = np.zeros((self.height, self.width), dtype=np.int8)
        self._call("read_denoise_guides_specular", specular_bounces, a.ctypes.data, n.ctypes.data, p.ctypes.data, chain.ctypes.data)
        return {"albedo": a, "normal": n, "position": p, "hit": chain != 0, "chain": chain}

    def GetDenoiseSpecular(self) -> dict:
        """Of the last call with specular_bounces: have (0 / 1), bounces, chain_ms (HIP-event milliseconds of the chain stage alone), rays,
        pixels_followed, pixels_escaped, pixels_truncated, and device_bytes of what the chain keeps (several devices: sums, the slowest device's time)."""
        out = N.DenoiseSpecular()
        self._call("get_denoise_specular", C.byref(out))
        return out.as_dict()

    def ReadDenoiseVirtual(self) -> dict:
        """Of the last Denoise(temporal=True, follow_specular=K): virtual_position (H x W x 3 float32: the virtual point of every pixel whose chain ended
        on a surface, the position guide of every other) and distance (H x W float32: the unfolded length; 0 where the pixel is not followed or the
        length is not a positive finite number)."""
        p = np.zeros((self.height, self.width, 3), dtype=np.float32)
        dist = np.zeros((self.height, self.width), dtype=np.float32)
        self._call("read_denoise_virtual", p.ctypes.data, dist.ctypes.data)
        return {"virtual_position": p, "distance": dist}

    def GetDenoiseVirtual(self) -> dict:
        """have (0 / 1), bounces, pixels_followed (class >= 2) and pixels_with_history (of them, those that took history) of the last
        Denoise(temporal=True, follow_specular=K), and device_bytes of what it keeps (several devices: summed)."""
        out = N.DenoiseVirtual()
        self._call("get_denoise_virtual", C.byref(out))
        return out.as_dict()

    def GetDenoiseTiming(self) -> dict:
        """HIP-event milliseconds of the last Denoise() on the (first) device: guides (0 with several devices: the upload instead), prepare, levels.
        After Denoise(temporal=True) the merge kernel's time is in none of the entries, so `total` leaves it out: add GetDenoiseMergeMs()."""
        ms = (C.c_float * 16)()
        c = self._contexts()[0]
        n = N.lib.adypt_get_denoise_timing(c, ms, 16)
        if n < 0:
            N.check(n, c)
        return {"guides": ms[0], "prepare": ms[1], "levels": [ms[i] for i in range(2, n)], "total": sum(ms[i] for i in range(n))}

    # ---- moving geometry (adypt_update_triangles, include/adypt_hip.h; the definition: csrc/device/refit.hpp) ----
    def UpdateTriangles(self, first: int, positions: np.ndarray, normals: Optional[np.ndarray] = None, rebuild_above: Optional[float] = None,
                        method: str = "ploc", radius: int = 8, split_budget: float = 0.0, cfg: Optional[N.BvhParams] = None) -> Optional[dict]:
        """New positions (count x 9 float32: p0 p1 p2) and, when given, normals (count x 9) of triangles [first, first + count); every reference's Woop
        data and every node are then refitted on the GPU.  Leaves the tracer as Reset() does (0 spp).  Several devices: on every device.
        rebuild_above None: that is all, and None is returned.  A number (adypt_update_triangles_auto): the SAH cost of the refitted tree is measured
        (GetTreeCost) and, where it is more than rebuild_above times the cost the tree had as uploaded or as last rebuilt, the tree is rebuilt as
        RebuildBVH(cfg, method, radius, split_budget) would; 0 always rebuilds, and there is no default (README, Moving geometry).  Returns built,
        refitted and now (each as GetTreeCost gives it), rebuilt (0 / 1), rebuild (RebuildBVH's dict; zeros when kept) and cost_ms."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 9)
        nrm = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 9)
        if nrm is not None and len(nrm) != len(pos):
            raise ValueError("UpdateTriangles: positions and normals differ in length")
        if rebuild_above is None:
            self._call("update_triangles", first, len(pos), pos.ctypes.data, None if nrm is None else nrm.ctypes.data)
            return None
        return self._under_policy("UpdateTriangles", "update_triangles_auto", (first, len(pos), pos.ctypes.data, None if nrm is None else nrm.ctypes.data),
                                  rebuild_above, cfg, method, radius, split_budget)

    def _under_policy(self, who: str, name: str, args: tuple, rebuild_above: float, cfg: Optional[N.BvhParams], method: str, radius: int, split_budget: float) -> dict:
        """adypt_update_triangles_auto / adypt_pose with the policy that the last five arguments make: the outcome"""
        params, *build = _build_args(who, cfg, method, radius, split_budget)
        policy, out = N.PosePolicy(float(rebuild_above), *build), N.PoseOutcome()
        self._call(name, *args, params, C.byref(policy), C.byref(out))
        return out.as_dict()

    # ---- posing on the GPU (adypt_bind_parts, adypt_bind_skin, adypt_pose, include/adypt_hip.h; the definition: csrc/device/pose.hpp) ----
    def BindParts(self, parts: np.ndarray, n_parts: Optional[int] = None) -> None:
        """Every triangle belongs to one part (int32 [n], 0 <= part < n_parts; n_parts None: the largest index + 1).  The device keeps the triangles
        as they are NOW as the rest pose; Pose() then moves them by one 3x4 matrix per part.  Replaces an earlier binding; nothing changes when
        the call is refused.  Several devices: on every device."""
        p = np.ascontiguousarray(parts, dtype=np.int32).reshape(-1)
        if n_parts is None:
            n_parts = int(p.max()) + 1 if len(p) else 0
        self._call("bind_parts", p.ctypes.data, len(p), int(n_parts))

    def BindSkin(self, joints: np.ndarray, weights: np.ndarray, n_joints: int) -> None:
        """Every vertex follows up to four weighted joints: joints (integers below 65536) and weights (float32, finite, >= 0, used as given), each
        [n, 3, 4] — triangle, vertex, slot.  A slot of weight 0 is skipped, its joint may be anything.  Otherwise as BindParts()."""
        j, w = _skin_arrays("BindSkin", joints, weights)
        self._call("bind_skin", j.ctypes.data, w.ctypes.data, len(j), int(n_joints))

    def Pose(self, matrices: np.ndarray, rebuild_above: Optional[float] = None, method: str = "ploc", radius: int = 8, split_budget: float = 0.0,
             cfg: Optional[N.BvhParams] = None, *, morph_weights=None) -> Optional[dict]:
        """The bound triangles under row-major 3x4 matrices (float32 [n_parts or n_joints, 3, 4]: [r][0..2] linear, [r][3] translation), always from
        the rest pose: positions, and normals through the cofactor matrix, are written into the device's records by one kernel, then the tree is
        refitted as UpdateTriangles() refits it — only the matrices cross the bus.  pose_triangles() is the same arithmetic on the host, bit for
        bit.  rebuild_above and the arguments after it, and what is returned: as for UpdateTriangles().
        morph_weights (adypt_pose_morph): one weight per target of the layer BindMorph() bound, applied to the rest pose before the matrices; None
        is every weight 0, which gives the bytes of a binding without a layer."""
        m = _pose_matrices("Pose", matrices)
        name, args = "pose", (m.ctypes.data, len(m))
        if morph_weights is not None:
            w = _morph_weights(morph_weights)
            name, args = "pose_morph", args + (w.ctypes.data, len(w))
        if rebuild_above is None:
            self._call(name, *args, None, None, None)
            return None
        return self._under_policy("Pose", name, args, rebuild_above, cfg, method, radius, split_budget)

    def BindMorph(self, triangles: np.ndarray, targets: np.ndarray, deltas: np.ndarray, n_targets: Optional[int] = None) -> None:
        """Adds a morph layer (blend shapes) to the EXISTING BindParts() / BindSkin() binding: entry e moves triangle triangles[e] by deltas[e]
        ([n, 18] or [n, 2, 3, 3]: the deltas of p0 p1 p2, then of n0 n1 n2) times the weight of target targets[e] (n_targets None: the largest
        index + 1).  Entries in any order, at most one per (triangle, target); morph_diff() makes them from a target mesh.  Replaces an earlier
        layer; nothing changes when the call is refused.  BindParts(), BindSkin(), UnbindPose() and SetTriangles() drop the layer; rebuilds keep it."""
        t, k, d = _morph_arrays("BindMorph", triangles, targets, deltas)
        if n_targets is None:
            n_targets = int(k.max()) + 1 if len(k) else 0
        self._call("bind_morph", t.ctypes.data, k.ctypes.data, d.ctypes.data, len(t), int(n_targets))

    def UnbindMorph(self) -> None:
        """Gives the morph layer back; the rest pose and the matrix binding stay."""
        self._call("unbind_morph")

    def GetMorphBinding(self) -> dict:
        """n_targets (0: no layer), n_entries, n_tris_touched and device_bytes of the morph layer of the (first) device."""
        out = N.MorphBinding()
        self._call("get_morph_binding", C.byref(out))
        return out.as_dict()

    def UnbindPose(self) -> None:
        """Gives the rest pose and the binding back; the triangles stay as the last Pose() left them."""
        self._call("unbind_pose")

    def GetPoseBinding(self) -> dict:
        """kind (0 none, 1 parts, 2 skin), n_matrices, n_tris and device_bytes of the binding of the (first) device."""
        out = N.PoseBinding()
        self._call("get_pose_binding", C.byref(out))
        return out.as_dict()

    # ---- an indexed mesh posed by its vertices (adypt_bind_mesh, adypt_pose_vertices, include/adypt_hip.h; the definition: csrc/device/mesh.hpp) ----
    def BindMesh(self, indices: np.ndarray, n_vertices: Optional[int] = None) -> None:
        """Every triangle corner names a vertex (int32 [n, 3], 0 <= index < n_vertices; n_vertices None: the largest index + 1).  PoseVertices()
        then moves the mesh by one position per vertex.  No rest pose is captured.  Replaces an earlier mesh binding and is independent of
        BindParts() / BindSkin(); nothing changes when the call is refused.  weld_triangles() makes the indices of a soup.  Several devices: on
        every device."""
        i, nv = _mesh_indices("BindMesh", indices, n_vertices)
        self._call("bind_mesh", i.ctypes.data, len(i), nv)

    def PoseVertices(self, positions: np.ndarray, normals: Optional[np.ndarray] = None, rebuild_above: Optional[float] = None, method: str = "ploc",
                     radius: int = 8, split_budget: float = 0.0, cfg: Optional[N.BvhParams] = None) -> Optional[dict]:
        """The bound mesh at new vertex positions (float32 [n_vertices, 3]) and, when given, vertex normals (used as given): 12 or 24 bytes per
        vertex cross the bus, the device writes positions and normals into every triangle's record and refits as UpdateTriangles() does.
        normals None: smooth normals are computed on the device (area-weighted, summed per vertex in a fixed order).  mesh_triangles() is the
        same arithmetic on the host, bit for bit.  rebuild_above and the arguments after it, and what is returned: as for UpdateTriangles()."""
        p = _vertex_array("PoseVertices", positions)
        nrm = None if normals is None else _vertex_array("PoseVertices", normals)
        if nrm is not None and len(nrm) != len(p):
            raise ValueError("PoseVertices: positions and normals differ in length")
        args = (p.ctypes.data, None if nrm is None else nrm.ctypes.data, len(p))
        if rebuild_above is None:
            self._call("pose_vertices", *args, None, None, None)
            return None
        return self._under_policy("PoseVertices", "pose_vertices", args, rebuild_above, cfg, method, radius, split_budget)

    def ReadVertexNormals(self) -> np.ndarray:
        """float32 [n_vertices, 3]: the vertex normals of the last PoseVertices(), computed or given, as the (first) device holds them."""
        out = np.empty((self.GetMeshBinding()["n_vertices"], 3), dtype=np.float32)
        self._call("read_vertex_normals", out.ctypes.data)
        return out

    def GetMeshTiming(self) -> dict:
        """HIP-event milliseconds of the stages of the last PoseVertices() on the (first) device: upload, faces, normals (both 0 with given
        normals), records.  Together they are GetRefitTiming()'s "scatter"."""
        ms = (C.c_float * 4)()
        c = self._contexts()[0]
        n = N.lib.adypt_get_mesh_timing(c, ms, 4)
        if n < 0:
            N.check(n, c)
        return {"upload": ms[0], "faces": ms[1], "normals": ms[2], "records": ms[3]}

    def UnbindMesh(self) -> None:
        """Gives the mesh binding back; the triangles stay as the last PoseVertices() left them."""
        self._call("unbind_mesh")

    def GetMeshBinding(self) -> dict:
        """n_vertices (0: none), n_tris, max_valence and device_bytes of the mesh binding of the (first) device."""
        out = N.MeshBinding()
        self._call("get_mesh_binding", C.byref(out))
        return out.as_dict()

    def GetTreeCost(self, cfg: Optional[N.BvhParams] = None) -> dict:
        """adypt_get_tree_cost: WideBVH.Cost() of the tree the device holds now, measured there by one pass over the nodes — cost, inner_q, leaf_q,
        n_nodes.  Several devices: every device measures, and all must agree."""
        out = N.TreeCost()
        self._call("get_tree_cost", None if cfg is None else C.byref(cfg), C.byref(out))
        return out.as_dict()

    def ReadBVH(self) -> Tuple[np.ndarray, np.ndarray]:
        """(nodes uint8 [n_nodes * 80], woop float32 [n_refs, 12]) as they are on the (first) device."""
        c = self._contexts()[0]
        n_nodes, n_refs = self.GetBVHSizes()
        nodes, woop = np.zeros(n_nodes * NODE_BYTES, dtype=np.uint8), np.zeros((n_refs, 12), dtype=np.float32)
        N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, woop.ctypes.data), c)
        return nodes, woop

    def ReadRootCard(self) -> np.ndarray:
        """The root card of the (first) device as it is now: one ROOT_CARD_DT record (adypt_read_root_card; csrc/device/root_card.hpp)."""
        c = self._contexts()[0]
        card = np.zeros(1, dtype=ROOT_CARD_DT)
        N.check(N.lib.adypt_read_root_card(c, card.ctypes.data), c)
        return card[0]

    # ---- rebuilding the tree on the GPU (adypt_rebuild_bvh, include/adypt_hip.h; the definition: csrc/device/lbvh.hpp) ----
    def RebuildBVH(self, cfg: Optional[N.BvhParams] = None, method: str = "linear", radius: int = 8, split_budget: float = 0.0) -> dict:
        """A new tree, built on the GPU from the triangles as UpdateTriangles() left them.  method "linear": WideBVH.BuildLinear's bytes; "ploc": those
        of WideBVH.BuildPLOC(radius=radius) — a tighter tree on meshes for a few times the build time (csrc/device/ploc.hpp); radius counts for "ploc"
        only.  split_budget in [0, 1], for "ploc" only: large triangles are split into several references first, at most split_budget * n more than
        triangles (csrc/device/presplit.hpp; WideBVH.BuildPLOC(split_budget=...)'s bytes; GetRebuildPresplit(), ReadRefBoxes()) — for scenes with
        large triangles among small ones; rebuild such a tree for a new pose rather than refitting it.  Leaves the tracer as Reset() does (0 spp).  Several devices: on every device.  Returns n_nodes, n_refs, levels (size stack_size by it)
        and binary_depth."""
        params, ploc, radius, split_budget = _build_args("RebuildBVH", cfg, method, radius, split_budget)
        info = N.RebuildInfo()
        if ploc and split_budget != 0.0:
            self._call("rebuild_bvh_ploc_split", params, radius, split_budget, C.byref(info))
        elif ploc:
            self._call("rebuild_bvh_ploc", params, radius, C.byref(info))
        else:
            self._call("rebuild_bvh", params, C.byref(info))
        return info.as_dict()

    # ---- replacing the triangles on the GPU (adypt_set_triangles, include/adypt_hip.h; the record: csrc/device/tri_record.hpp) ----
    def SetTriangles(self, triangles: np.ndarray, cfg: Optional[N.BvhParams] = None, method: str = "ploc", radius: int = 8, split_budget: float = 0.0) -> dict:
        """Replaces ALL triangles by the given ones (uint8, n x 100 bytes as Scene.GetTriangles() gives them; any n >= 1) and builds their tree on the
        GPU as RebuildBVH(cfg, method, radius, split_budget) would; materials and textures (SetMaterials changes those), camera and configuration stay.  Nothing changes when the call
        is refused or fails.  Leaves the tracer as Reset() does (0 spp).  Several devices: on every device.  Returns RebuildBVH's dict."""
        info = N.RebuildInfo()
        self._call("set_triangles", *_set_triangles_args("SetTriangles", triangles, cfg, method, radius, split_budget), C.byref(info))
        return info.as_dict()

    # ---- materials, textures and triangle attributes changed on the GPU (adypt_set_materials ..., include/adypt_hip.h; csrc/device/appearance.hpp) ----
    def SetMaterials(self, materials, textures=None) -> dict:
        """Replaces the material table (uint8, n x 64 bytes as Scene.GetMaterials() gives them; any n >= 0) and, unless textures is None, ALL textures
        (a sequence of uint8 [h, w, 3], possibly empty); every triangle is classified again.  Nothing changes when the call is refused or fails.
        Leaves the tracer as UpdateTriangles() does (0 spp); tree, bindings and the denoiser's history stay.  Several devices: on every device.
        Returns GetAppearance()."""
        m = _materials_array("SetMaterials", materials)
        tex, n_tex, keep = (None, -1, None) if textures is None else _texture_table("SetMaterials", textures)
        self._call("set_materials", m.ctypes.data if len(m) else None, len(m) // MAT_BYTES, tex, n_tex)
        del keep
        return self.GetAppearance()

    def UpdateTexture(self, index: int, rgb) -> dict:
        """New texels (uint8 [h, w, 3]) for texture `index`, in place: the size must be the texture's own (another size: SetMaterials).  Leaves the
        tracer at 0 spp.  Returns GetAppearance()."""
        t = np.ascontiguousarray(rgb, dtype=np.uint8)
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("UpdateTexture: a texture is uint8 [height, width, 3]")
        self._call("update_texture", int(index), t.ctypes.data if t.size else None, t.shape[1], t.shape[0])
        return self.GetAppearance()

    def SetTriangleAttributes(self, first: int, material_ids=None, texcoords=None) -> dict:
        """Material ids (int32 [count]) and/or texture coordinates (float32 [count, 6]) for the triangles from `first` on; class words follow the ids.
        Ids are not checked (a bad id renders as a bad material and is counted).  Leaves the tracer at 0 spp.  Returns GetAppearance(), whose
        'reclassed' counts the triangles whose class word changed."""
        ids = None if material_ids is None else np.ascontiguousarray(material_ids, dtype=np.int32).reshape(-1)
        uv = None if texcoords is None else np.ascontiguousarray(texcoords, dtype=np.float32).reshape(-1, 6)
        if ids is not None and uv is not None and len(ids) != len(uv):
            raise ValueError("SetTriangleAttributes: %d material ids and %d sets of texture coordinates" % (len(ids), len(uv)))
        count = len(ids) if ids is not None else len(uv) if uv is not None else 0
        self._call("set_triangle_attributes", int(first), count, None if ids is None else ids.ctypes.data, None if uv is None else uv.ctypes.data)
        return self.GetAppearance()

    def GetAppearance(self) -> dict:
        """adypt_appearance_info of the (first) device: counts, device bytes, and of the last setter the reclassified triangles and its stage times."""
        c = self._contexts()[0]
        info = N.AppearanceInfo()
        N.check(N.lib.adypt_get_appearance(c, C.byref(info)), c)
        return info.as_dict()

    def ReadMaterialRecords(self) -> np.ndarray:
        """The 80-byte material records of the (first) device (uint32 [n_mats, 20])."""
        c = self._contexts()[0]
        rec = np.zeros((self.GetAppearance()["n_mats"], 20), dtype=np.uint32)
        N.check(N.lib.adypt_read_material_records(c, rec.ctypes.data if len(rec) else np.zeros(1, np.uint32).ctypes.data), c)
        return rec

    def ReadTexels(self) -> np.ndarray:
        """The texture arena of the (first) device (uint32 [n_texels]): rows of w + 1 RGBA8 words (pack_appearance)."""
        c = self._contexts()[0]
        out = np.zeros(max(1, self.GetAppearance()["n_texels"]), dtype=np.uint32)
        N.check(N.lib.adypt_read_texels(c, out.ctypes.data), c)
        return out[:self.GetAppearance()["n_texels"]]

    def GetTriangleCount(self) -> int:
        """The triangles the (first) device holds now."""
        c = self._contexts()[0]
        n = N.lib.adypt_get_triangle_count(c)
        if n < 0:
            N.check(int(n), c)
        return int(n)

    def ReadTriangles(self) -> np.ndarray:
        """The triangles as they are on the (first) device, in Scene.GetTriangles()'s layout (uint8 [n * 100]): unpacked from the 128-byte records."""
        c = self._contexts()[0]
        rec = np.zeros((self.GetTriangleCount(), 32), dtype=np.uint32)
        N.check(N.lib.adypt_read_triangle_records(c, rec.ctypes.data), c)
        return np.ascontiguousarray(np.concatenate([rec[:, 0:18], rec[:, 20:26], rec[:, 18:19]], axis=1)).view(np.uint8).reshape(-1)

    def ReadTriangleRecords(self) -> np.ndarray:
        """The raw 128-byte records of the (first) device (uint32 [n, 32])."""
        c = self._contexts()[0]
        rec = np.zeros((self.GetTriangleCount(), 32), dtype=np.uint32)
        N.check(N.lib.adypt_read_triangle_records(c, rec.ctypes.data), c)
        return rec

    def GetSetTrianglesTiming(self) -> dict:
        """HIP-event milliseconds of the last SetTriangles() on the (first) device, in front of what GetRebuildTiming() gives for its build."""
        ms = (C.c_float * 3)()
        c = self._contexts()[0]
        n = N.lib.adypt_get_set_triangles_timing(c, ms, 3)
        if n < 0:
            N.check(n, c)
        return {"stage": ms[0], "pack": ms[1], "total": ms[2]}

    def GetBVHSizes(self) -> Tuple[int, int]:
        """(n_nodes, n_refs) of the tree the (first) device holds now."""
        n_nodes, n_refs = C.c_int64(), C.c_int64()
        c = self._contexts()[0]
        N.check(N.lib.adypt_get_bvh_sizes(c, C.byref(n_nodes), C.byref(n_refs)), c)
        return n_nodes.value, n_refs.value

    def ReadTriIndices(self) -> np.ndarray:
        """The reference order (int32 [n_refs]) as it is on the (first) device."""
        idx = np.zeros(max(self.GetBVHSizes()[1], 1), dtype=np.int32)
        c = self._contexts()[0]
        N.check(N.lib.adypt_read_tri_indices(c, idx.ctypes.data), c)
        return idx[:self.GetBVHSizes()[1]]

    def GetRebuildPresplit(self) -> Tuple[int, int]:
        """(the level of detail the last RebuildBVH() chose, -1 for none; the triangles it split) on the (first) device."""
        out = (C.c_int32 * 2)()
        c = self._contexts()[0]
        N.check(N.lib.adypt_get_rebuild_presplit(c, out), c)
        return out[0], out[1]

    def ReadRefBoxes(self) -> Optional[np.ndarray]:
        """The reference boxes (float32 [n_refs, 6]: lo xyz, hi xyz) of a tree rebuilt with split_budget as they are on the (first) device, in the
        order of ReadTriIndices(); None when the tree has none (not built with splits, or refitted since)."""
        c = self._contexts()[0]
        n = N.lib.adypt_read_ref_boxes(c, None)
        if n < 0:
            N.check(int(n), c)
        if n == 0:
            return None
        out = np.zeros((n, 6), dtype=np.float32)
        n = N.lib.adypt_read_ref_boxes(c, out.ctypes.data)
        if n < 0:
            N.check(int(n), c)
        return out

    def GetRebuildTiming(self) -> dict:
        """HIP-event milliseconds of the last RebuildBVH() on the (first) device.  After method "ploc": "tree" is all the rounds, "bottom_up" is 0."""
        ms = (C.c_float * 7)()
        c = self._contexts()[0]
        n = N.lib.adypt_get_rebuild_timing(c, ms, 7)
        if n < 0:
            N.check(n, c)
        return dict(zip(("keys", "sort", "tree", "bottom_up", "emission", "woop_nodes", "total"), (ms[i] for i in range(7))))

    def GetRefitTiming(self) -> dict:
        """HIP-event milliseconds of the last UpdateTriangles() on the (first) device."""
        ms = (C.c_float * 4)()
        c = self._contexts()[0]
        n = N.lib.adypt_get_refit_timing(c, ms, 4)
        if n < 0:
            N.check(n, c)
        return {"scatter": ms[0], "references_woop": ms[1], "nodes": ms[2], "total": ms[3]}

    def ReadDisplay(self) -> np.ndarray:
        """What OglPathTracer::DrawScreen puts on screen (shaders/screen.glsl:15-21): H x W x 4 uint8; every context converts its own tiles."""
        rgba = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._call("read_display", rgba.ctypes.data)
        return rgba

    def ReadResult(self) -> np.ndarray:
        rgb = np.zeros((self.height, self.width, 3), dtype=np.float32)
        self._call("read_radiance", rgb.ctypes.data)
        return rgb

    def SaveResult(self, filename: str, save_as_fp16: bool) -> None:
        save_exr(filename, self.ReadResult(), save_as_fp16)

    def destroy(self) -> None:
        if self._h:
            getattr(N.lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:
        try:
            self.destroy()
        except Exception:
            pass


class HipPathTracer(_Tracer):
    """OglPathTracer (src/Tracer/OglPathTracer.hpp:66-82) on HIP."""
    _family, _destroy = "adypt_", "adypt_destroy"
    _ctx = property(lambda self: self._h)

    def _check(self, code: int) -> None:
        N.check(code, self._h)

    def _contexts(self):
        return [self._h]

    def Initialize(self, config: N.PtParams, scene: HipScene, width: int, height: int, device: int = 0,
                   tile_rank: int = 0, tile_nranks: int = 1, method: str = "ploc", radius: int = 8, split_budget: float = 0.0,
                   cfg: Optional[N.BvhParams] = None) -> None:
        """A scene without a BVH (HipScene.Initialize(scene)): the first tree is built on the GPU as SetTriangles(cfg=cfg, method=method, radius=radius,
        split_budget=split_budget) builds it, and build_info is what that returns; with a BVH those four are not looked at and build_info is None."""
        self.destroy()
        self.width, self.height = width, height
        self.tile_rank, self.tile_nranks = tile_rank, tile_nranks
        d, self._keep = _scene_desc(scene, width, height)
        d.device, d.tile_rank, d.tile_nranks = device, tile_rank, tile_nranks
        self.build_info = None
        if scene.bvh is None:
            info = N.RebuildInfo()
            args = _set_triangles_args("HipPathTracer.Initialize", scene.scene.triangles, cfg, method, radius, split_budget)[2:]
            N.check(N.lib.adypt_create_from_triangles(C.byref(self._h), C.byref(d), *args, C.byref(info)))
            self.build_info = info.as_dict()
        else:
            N.check(N.lib.adypt_create(C.byref(self._h), C.byref(d)))
        self.SetConfig(config)

    def TraceAsync(self, n_spp: int = 1) -> None:
        """Trace(true) n_spp times without waiting for the GPU (adypt_trace_spp_async); pair with Wait()."""
        self.m_viewer_type = ViewerTypes.kPTRadiance
        N.check(N.lib.adypt_trace_spp_async(self._ctx, n_spp), self._ctx)

    def Wait(self) -> None:
        N.check(N.lib.adypt_wait(self._ctx), self._ctx)

    def SetFramesInFlight(self, n: int) -> None:
        N.check(N.lib.adypt_set_frames_in_flight(self._ctx, n), self._ctx)

    def SetPipeline(self, n_pipes: int) -> None:
        """Sub-batches per batch, each a chain of kernels on its own HIP stream (adypt_set_pipeline); 1 = serial."""
        N.check(N.lib.adypt_set_pipeline(self._ctx, n_pipes), self._ctx)

    def GetPipeline(self) -> int:
        return N.lib.adypt_get_pipeline(self._ctx)

    def SetFusedBounces(self, enabled: bool) -> None:
        """Every bounce after the first of a batch in one launch (k_path); default on.  Images are bit-identical either way."""
        N.check(N.lib.adypt_set_fused_bounces(self._ctx, 1 if enabled else 0), self._ctx)

    def GetLookaheadFrames(self) -> int:
        return N.lib.adypt_get_lookahead_frames(self._ctx)

    def SavePreview(self, filename: str) -> None:
        save_png(filename, self.ReadDisplay())

    def ReadHits(self) -> Tuple[np.ndarray, np.ndarray]:
        tri = np.full((self.height, self.width), -1, dtype=np.int32)
        uv = np.zeros((self.height, self.width, 2), dtype=np.float32)
        N.check(N.lib.adypt_read_hits(self._ctx, tri.ctypes.data, uv.ctypes.data), self._ctx)
        return tri, uv

    def TraceRays(self, rays: np.ndarray, with_stats: bool = True, any_hit: bool = False) -> np.ndarray:
        """closest-hit batch (traversal.glsl:14-255) or, with any_hit, the occlusion overload (traversal.glsl:257-494)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        hits = np.zeros(len(rays), dtype=HIT_DT)
        fn = N.lib.adypt_trace_rays_any if any_hit else N.lib.adypt_trace_rays
        N.check(fn(self._ctx, rays.ctypes.data, len(rays), hits.ctypes.data, 1 if with_stats else 0), self._ctx)
        return hits

    def SetInstrumentation(self, timing: bool = False, counters: bool = False, audit: bool = False) -> None:
        """audit: the slot-claim audit of the ray queues (GetStats()["audit_errors"] must stay 0); a debugging aid, slow."""
        N.check(N.lib.adypt_set_instrumentation(self._ctx, (1 if timing else 0) | (2 if counters else 0) | (4 if audit else 0)), self._ctx)

    def GetWaveProfile(self) -> dict:
        out = (C.c_uint64 * 8)()
        N.check(N.lib.adypt_get_wave_profile(self._ctx, out), self._ctx)
        keys = ("trips", "trip_lanes", "tri_iters", "tri_lanes", "node_phases", "node_lanes", "refills", "empty_trips")
        return dict(zip(keys, [int(v) for v in out]))

    def local_pixel_count(self) -> int:
        return N.lib.adypt_local_pixel_count(self._ctx)

    def local_radiance_device_ptr(self) -> int:
        p = C.c_void_p()
        N.check(N.lib.adypt_local_radiance_device(self._ctx, C.byref(p)), self._ctx)
        return p.value

    def copy_local_radiance(self, dst_device_ptr: int, capacity_float4: int) -> None:
        N.check(N.lib.adypt_copy_local_radiance(self._ctx, dst_device_ptr, capacity_float4), self._ctx)

    def assemble_radiance(self, gathered_device_ptr: int, stride_float4: int, rgb_device_ptr: int) -> None:
        N.check(N.lib.adypt_assemble_radiance(self._ctx, gathered_device_ptr, stride_float4, rgb_device_ptr), self._ctx)

    # ---- one process per GPU: the library's own RCCL communicator (adypt_comm_*) ----
    def CommInit(self, unique_id: bytes) -> None:
        assert len(unique_id) == 128
        N.check(N.lib.adypt_comm_init(self._ctx, unique_id), self._ctx)

    def CommGatherDevice(self) -> Optional[int]:
        """Collective: the one gather.  Rank 0 gets the device pointer of the assembled W x H x 3 fp32 image, the others None."""
        p = C.c_void_p()
        N.check(N.lib.adypt_comm_gather_radiance(self._ctx, C.byref(p)), self._ctx)
        return p.value

    def CommReadResult(self) -> Optional[np.ndarray]:
        """Collective: gather + device-to-host copy on rank 0 (None elsewhere)."""
        rgb = np.zeros((self.height, self.width, 3), dtype=np.float32) if self.tile_rank == 0 else None
        N.check(N.lib.adypt_comm_read_radiance(self._ctx, None if rgb is None else rgb.ctypes.data), self._ctx)
        return rgb

    def CommAllReduce(self, values, op: str = "sum"):
        arr = (C.c_double * len(values))(*[float(v) for v in values])
        N.check(N.lib.adypt_comm_allreduce(self._ctx, arr, len(values), {"sum": 0, "max": 1}[op]), self._ctx)
        return [float(v) for v in arr]

    def CommBarrier(self) -> None:
        N.check(N.lib.adypt_comm_barrier(self._ctx), self._ctx)


class MultiPathTracer(_Tracer):
    """One host process driving N GPUs through the library's own multi-device boundary (adypt_create_multi): tile rank i on
    devices[i], scene replicated, the radiance gathered on devices[0] with RCCL inside adypt_multi_read_radiance.  Same method
    names as HipPathTracer / OglPathTracer."""
    _family, _destroy = "adypt_multi_", "adypt_destroy_multi"
    _m = property(lambda self: self._h)

    def _check(self, code: int) -> None:
        if code != N.ADYPT_OK:
            msg = N.lib.adypt_multi_last_error(self._h if self._h else None)
            raise N.AdyptError(code, (msg or b"").decode("utf-8", "replace"))

    def _contexts(self):
        return [N.lib.adypt_multi_context(self._m, i) for i in range(self.DeviceCount())]

    def Initialize(self, config: N.PtParams, scene: HipScene, width: int, height: int, devices: Sequence[int] = (0,), method: str = "ploc", radius: int = 8,
                   split_budget: float = 0.0, cfg: Optional[N.BvhParams] = None) -> None:
        """A scene without a BVH: as HipPathTracer.Initialize, every device building its own copy of the tree (adypt_create_multi_from_triangles)."""
        self.destroy()
        self.width, self.height = width, height
        d, self._keep = _scene_desc(scene, width, height)
        devs = (C.c_int * len(devices))(*devices)
        self.build_info = None
        if scene.bvh is None:
            info = N.RebuildInfo()
            args = _set_triangles_args("MultiPathTracer.Initialize", scene.scene.triangles, cfg, method, radius, split_budget)[2:]
            self._check(N.lib.adypt_create_multi_from_triangles(C.byref(self._h), C.byref(d), devs, len(devices), *args, C.byref(info)))
            self.build_info = info.as_dict()
        else:
            self._check(N.lib.adypt_create_multi(C.byref(self._h), C.byref(d), devs, len(devices)))
        self.SetConfig(config)

    def SetupSeconds(self, i: int) -> float:
        """Seconds adypt_create took for devices[i] (the contexts are created concurrently, one host thread each)."""
        return float(N.lib.adypt_multi_setup_seconds(self._m, i))

    def CommInit(self) -> None:
        self._check(N.lib.adypt_multi_comm_init(self._m))

    def DeviceCount(self) -> int:
        return N.lib.adypt_multi_device_count(self._m)

    def SetInstrumentation(self, timing: bool = False, counters: bool = False) -> None:
        self._check(N.lib.adypt_multi_set_instrumentation(self._m, (1 if timing else 0) | (2 if counters else 0)))

    def ContextStats(self, i: int) -> dict:
        st = N.Stats()
        N.check(N.lib.adypt_get_stats(N.lib.adypt_multi_context(self._m, i), C.byref(st)))
        return st.as_dict()

    def GatherDevice(self) -> int:
        """Device pointer (on devices[0]) of the assembled W x H x 3 fp32 image; owned by the library."""
        p = C.c_void_p()
        self._check(N.lib.adypt_multi_gather_radiance(self._m, C.byref(p)))
        return p.value


class Instance:
    """Headless Instance (src/Instance.cpp): config -> scene -> (.bvh cache | build) -> upload -> tracer -> camera."""

    def __init__(self) -> None:
        self.m_config = InstanceConfig()
        self.m_path_tracer = HipPathTracer()
        self.m_hipscene = HipScene()
        self.m_camera = Camera()
        self.m_valid = False

    def InitializeFromFile(self, filename: str, shift_seed: int = 12345, device: int = 0, tile_rank: int = 0,
                           tile_nranks: int = 1, devices: Optional[Sequence[int]] = None, build_on_gpu: bool = False) -> bool:
        self.m_filename = filename
        if not self.m_config.LoadFromFile(filename):
            return False
        return self.Initialize(shift_seed, device, tile_rank, tile_nranks, devices, build_on_gpu)

    def Initialize(self, shift_seed: int = 12345, device: int = 0, tile_rank: int = 0, tile_nranks: int = 1,
                   devices: Optional[Sequence[int]] = None, build_on_gpu: bool = False) -> bool:
        """build_on_gpu: no .bvh cache is read or written and no host build runs; the tracer builds the first tree on the GPU (PLOC, radius 8) with the
        configuration's SAH costs.
        devices: a list of HIP device ordinals -> ONE process drives all of them through adypt_create_multi (tile rank i on
        devices[i]; m_path_tracer is then a MultiPathTracer), as integration/HipPathTracer.hpp does for the reference's Instance."""
        cfg = self.m_config
        self.scene = Scene()
        if not self.scene.LoadFromFile(cfg.m_obj_filename):
            return False
        bp = cfg.bvh_params()
        self.bvh = None if build_on_gpu else WideBVH()
        if self.bvh is not None and not self.bvh.LoadFromFile(cfg.m_bvh_filename, bp):
            self.bvh.Build(self.scene, bp)
            if not self.bvh.SaveToFile(cfg.m_bvh_filename, bp):
                return False
        self.m_hipscene.Initialize(self.scene, self.bvh)
        if devices is not None:
            self.m_path_tracer = MultiPathTracer()
            self.m_path_tracer.Initialize(cfg.pt_params(shift_seed), self.m_hipscene, cfg.m_width, cfg.m_height, list(devices), cfg=bp)
        else:
            self.m_path_tracer.Initialize(cfg.pt_params(shift_seed), self.m_hipscene, cfg.m_width, cfg.m_height, device, tile_rank, tile_nranks, cfg=bp)
        self.m_camera.Initialize(cfg, cfg.m_width, cfg.m_height)
        ip, iv = self.m_camera.matrices()
        self.m_path_tracer.SetCamera(ip, iv, self.m_camera.position)
        self.m_valid = True
        return True

    def Update(self, enable_pt: bool, n_spp: int = 1, keys: int = 0, mouse: Tuple[float, float] = (0.0, 0.0),
               frame_seconds: float = 0.0) -> None:
        """Instance::Update (src/Instance.cpp:44-57) without the window: while not path tracing the camera follows the input
        state (Camera::Control) and is handed to the tracer, then one Trace(enable_pt)."""
        if not enable_pt:
            self.m_camera.Control(keys, mouse[0], mouse[1], frame_seconds)
            ip, iv = self.m_camera.matrices()
            self.m_path_tracer.SetCamera(ip, iv, self.m_camera.position)
        self.m_path_tracer.Trace(enable_pt, n_spp)
