"""csrc/device/mesh.hpp restated in numpy float32, bit for bit: the incidence lists, the face vectors, the ordered sum per vertex, the normalisation
and the record words — every numpy operation below is one binary32 operation per element, in the order the header writes them.  And the meshes the
mesh tests run on."""
import numpy as np

from oracle import oracle_py as O

F = np.float32


def incidence(indices, n_vertices):
    """(offsets int64 [n_vertices + 1], triangles int32 [3 n]): vertex v's list is triangles[offsets[v] : offsets[v + 1]], in ascending 3 t + c"""
    flat = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
    order = np.argsort(flat, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_vertices))]).astype(np.int64)
    return offsets, (order // 3).astype(np.int32)


def faces(indices, positions):
    i, p = np.asarray(indices).reshape(-1, 3), np.ascontiguousarray(positions, dtype=F).reshape(-1, 3)
    p0, p1, p2 = p[i[:, 0]], p[i[:, 1]], p[i[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    with np.errstate(all="ignore"):
        return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def sums(indices, positions):
    """(acc float32 [n_vertices, 3], valence): the face vectors of every vertex's list added in list order, the first one taken as it is"""
    nv = len(np.asarray(positions).reshape(-1, 3))
    f = faces(indices, positions)
    offsets, tri = incidence(indices, nv)
    valence = np.diff(offsets)
    acc = np.zeros((nv, 3), F)
    with np.errstate(all="ignore"):
        for k in range(int(valence.max()) if nv else 0):
            has = np.nonzero(valence > k)[0]
            fk = f[tri[offsets[has] + k]]
            acc[has] = fk if k == 0 else acc[has] + fk
    return acc, valence


def normalise(acc):
    with np.errstate(all="ignore"):
        len2 = (acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2]
        ok = (len2 > 0) & (len2 < np.inf)
        n = acc.copy()
        n[ok] = acc[ok] / np.sqrt(len2[ok])[:, None]
    return n, ok


def normals(indices, positions):
    return normalise(sums(indices, positions)[0])[0]


def triangles(tris, indices, positions, given=None):
    """TRI_DT: corner c of triangle t takes the position and the normal (given, or computed) of vertex indices[t, c]; everything else stays"""
    i = np.asarray(indices).reshape(-1, 3)
    p = np.ascontiguousarray(positions, dtype=F).reshape(-1, 3)
    n = normals(i, p) if given is None else np.ascontiguousarray(given, dtype=F).reshape(-1, 3)
    t = np.ascontiguousarray(tris).view(O.TRI_DT).reshape(-1).copy()
    t["p"], t["n"] = p[i], n[i]
    return t


def referenced(indices, n_vertices):
    return np.bincount(np.asarray(indices).reshape(-1), minlength=n_vertices) > 0


# ---- the meshes: (indices int32 [n, 3], positions float32 [n_vertices, 3]) ----
def fan(k):
    """k triangles around an apex (vertex 0, valence k), k + 2 vertices, the rim bent out of the plane"""
    a = np.linspace(0.0, 5.5, k + 1)
    r = 2.0 + 0.5 * np.cos(5.0 * a)
    rim = np.stack([r * np.cos(a), 0.6 * np.sin(3.0 * a) + 0.1 * a, r * np.sin(a)], axis=1)
    p = np.concatenate([[[0.1, 1.2, -0.2]], rim]).astype(F)
    t = np.arange(k, dtype=np.int32)
    return np.stack([np.zeros(k, np.int32), t + 2, t + 1], axis=1), p


def grid(w, h):
    """2 w h triangles over (w + 1) x (h + 1) vertices, the heights from a fixed RandomState; an interior vertex has valence 6"""
    rs = np.random.RandomState(1000 * w + h)
    x, z = np.meshgrid(np.arange(w + 1), np.arange(h + 1))
    p = np.stack([0.5 * x.ravel() - 0.25 * w, rs.uniform(-0.4, 0.4, size=x.size), 0.5 * z.ravel() - 0.25 * h], axis=1).astype(F)
    c = (np.arange(h)[:, None] * (w + 1) + np.arange(w)[None, :]).ravel().astype(np.int32)
    a, b, d, e = c, c + 1, c + w + 1, c + w + 2
    i = np.concatenate([np.stack([a, d, b], axis=1), np.stack([b, d, e], axis=1)]).astype(np.int32)
    return i.reshape(2, -1, 3).transpose(1, 0, 2).reshape(-1, 3).copy(), p


def opposite_pair():
    """(a, b, c) and (a, c, b): every vertex's sum cancels, so its normal stays the unnormalised sum, the signs of its zeros included"""
    p = np.array([[0.5, -0.25, 0.0], [-1.0, 0.5, 0.0], [0.25, 2.0, 0.0]], F)
    return np.array([[0, 1, 2], [0, 2, 1]], np.int32), p


def with_unreferenced():
    """fan(5) with one more vertex, number 3, that no triangle names"""
    i, p = fan(5)
    return (i + (i >= 3)).astype(np.int32), np.insert(p, 3, [7.0, 7.0, 7.0], axis=0).astype(F)


def with_doubled_index():
    """fan(4) and one more triangle that names vertex 1 twice: its face vector is 0"""
    i, p = fan(4)
    return np.concatenate([i, [[1, 1, 2]]]).astype(np.int32), p


def rest_triangles(indices, positions):
    """TRI_DT of the mesh with computed normals, texture coordinates and material ids (0, and -1 on every third) that a pose must keep"""
    n = len(indices)
    t = np.zeros(n, dtype=O.TRI_DT)
    t["tc"] = np.random.RandomState(n).uniform(size=t["tc"].shape).astype(F)
    t["matid"] = np.where(np.arange(n) % 3 == 2, -1, 0)
    return triangles(t, indices, positions)


def deform(positions, seed=1):
    """every vertex somewhere else: a wave and a little noise"""
    p = np.ascontiguousarray(positions, dtype=F).reshape(-1, 3).astype(np.float64)
    rs = np.random.RandomState(seed)
    p[:, 1] += 0.5 * np.sin(0.9 * p[:, 0] + seed) + 0.3 * np.cos(1.3 * p[:, 2])
    p[:, 0] *= 1.0 + 0.05 * seed
    return (p + rs.normal(0, 0.05, size=p.shape)).astype(F)


def some_normals(n_vertices, seed=2):
    """vectors of any length: given normals are used as given"""
    return np.random.RandomState(seed).normal(0, 1.5, size=(n_vertices, 3)).astype(F)
