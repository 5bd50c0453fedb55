"""The refit of a CWBVH8 (adypt_amd/csrc/device/refit.hpp) restated in numpy float32, whole arrays at a time: what adypt_bvh_refit and the device path
are held against, bit for bit.  Not a translation of the header's loops: the unions are taken on integer keys that order the binary32 values (so that
-0 sorts below +0 and a minimum over any axis is the definition's), the levels come from a frontier walk over index arrays."""
import numpy as np

from oracle import oracle_py as O

INF_LO, INF_HI = np.float32(np.inf), np.float32(-np.inf)


def key(f):
    """binary32 -> int32, monotonic, -0 below +0"""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.int32)
    return np.where(u < 0, u ^ np.int32(0x7fffffff), u)


def unkey(k):
    k = np.asarray(k, dtype=np.int32)
    return np.where(k < 0, k ^ np.int32(0x7fffffff), k).astype(np.int32).view(np.float32)


def decode(nodes):
    """per slot [n, 8]: occupied, internal, child node index, leaf, first reference, number of references"""
    meta = nodes["meta"].astype(np.int64)
    occ = meta != 0
    inner = occ & ((meta >> 5) == 1) & ((meta & 31) >= 24)
    leaf = occ & ~inner
    child = nodes["child_base"].astype(np.int64)[:, None] + (meta & 31) - 24
    first = nodes["tri_base"].astype(np.int64)[:, None] + (meta & 31)
    count = np.select([(meta >> 5) == 1, (meta >> 5) == 3, (meta >> 5) == 7], [1, 2, 3], 0) * leaf
    return occ, inner, child, leaf, first, count


def depths(nodes):
    _, inner, child, _, _, _ = decode(nodes)
    depth = np.full(len(nodes), -1, dtype=np.int64)
    frontier, d = np.array([0]), 0
    while len(frontier):
        assert (depth[frontier] == -1).all(), "a node is reached twice"
        depth[frontier] = d
        frontier, d = child[frontier][inner[frontier]], d + 1
    assert (depth >= 0).all(), "a node is not reached"
    return depth


def exponent_byte(cell):
    u = np.ascontiguousarray(cell, dtype=np.float32).view(np.uint32)
    e = ((u >> 23) & 255).astype(np.int64) + ((u & 0x7fffff) != 0)
    return np.where(cell == 0, 0, np.clip(e, 1, 254)).astype(np.uint32)


def quantise(x, e, up):
    scale = (e << 23).astype(np.uint32).view(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = (x.astype(np.float32) / scale).astype(np.float32)
        r = np.where(q < 255, np.ceil(q) if up else np.floor(q), 255)
        return np.where((e == 0) | np.isnan(r), 0, r).astype(np.uint8)


def refit(nodes, tri_indices, triangles):
    """(refitted NODE_DT array, exact node boxes lo [n, 3], hi [n, 3], exact slot boxes lo [n, 8, 3], hi [n, 8, 3])"""
    nodes = np.ascontiguousarray(nodes).view(O.NODE_DT).reshape(-1).copy()
    idx = np.asarray(tri_indices, dtype=np.int64)
    p = np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1)["p"]          # [T, vertex, axis]
    tlo, thi = key(p).min(axis=1), key(p).max(axis=1)                             # [T, axis]
    occ, inner, child, leaf, first, count = decode(nodes)
    n = len(nodes)
    slo = np.full((n, 8, 3), key(INF_LO), dtype=np.int32)
    shi = np.full((n, 8, 3), key(INF_HI), dtype=np.int32)
    for r in range(3):
        m = count > r
        t = idx[first[m] + r]
        slo[m] = np.minimum(slo[m], tlo[t])
        shi[m] = np.maximum(shi[m], thi[t])
    depth = depths(nodes)
    nlo, nhi = np.zeros((n, 3), dtype=np.int32), np.zeros((n, 3), dtype=np.int32)
    for d in range(int(depth.max()), -1, -1):
        at = np.nonzero(depth == d)[0]
        m = inner[at]
        rows = np.broadcast_to(at[:, None], m.shape)[m]
        cols = np.broadcast_to(np.arange(8)[None, :], m.shape)[m]
        slo[rows, cols] = nlo[child[at][m]]
        shi[rows, cols] = nhi[child[at][m]]
        nlo[at], nhi[at] = slo[at].min(axis=1), shi[at].max(axis=1)
    lo, hi = unkey(nlo), unkey(nhi)
    any_occ = occ.any(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        cell = ((hi - lo).astype(np.float32) * np.float32(1.0 / 255)).astype(np.float32)
    e = exponent_byte(cell)                                                       # [n, axis]
    nodes["p"][any_occ] = lo[any_occ]
    nodes["e"][any_occ] = e[any_occ].astype(np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        dlo = (unkey(slo) - lo[:, None, :]).astype(np.float32)
        dhi = (unkey(shi) - lo[:, None, :]).astype(np.float32)
    qlo, qhi = quantise(dlo, e[:, None, :], False), quantise(dhi, e[:, None, :], True)
    for a, name in enumerate("xyz"):
        nodes["qlo" + name][occ] = qlo[..., a][occ]
        nodes["qhi" + name][occ] = qhi[..., a][occ]
    return nodes, lo, hi, unkey(slo), unkey(shi)


def slots_contain(nodes, node_lo, slo, shi):
    """Every occupied slot's dequantised box contains its exact box, in the node's own frame: qlo * 2^(e - 127) <= c.lo - p and qhi * 2^(e - 127) >=
    c.hi - p, where the differences are the binary32 ones the quantiser (and the builder) takes and the products are exact in binary64.  Held against
    the real-number difference instead, either side can be short by half an ulp of the coordinate — the rounding of that one subtraction, which the
    builder's own records show as well; the traversal tests slots in this frame too ((p - origin) * idir + q * (2^e * idir))."""
    nodes = np.ascontiguousarray(nodes).view(O.NODE_DT).reshape(-1)
    occ = nodes["meta"] != 0
    assert np.array_equal(nodes["p"][occ.any(axis=1)].view(np.uint32), np.ascontiguousarray(node_lo, dtype=np.float32)[occ.any(axis=1)].view(np.uint32))
    scale = np.ldexp(1.0, nodes["e"].astype(np.int64) - 127)                      # [n, axis]
    ok = np.ones(occ.shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a, name in enumerate("xyz"):
            base, s = nodes["p"][:, a][:, None], scale[:, a][:, None]
            ok &= nodes["qlo" + name].astype(np.float64) * s <= (slo[..., a] - base).astype(np.float32).astype(np.float64)
            ok &= nodes["qhi" + name].astype(np.float64) * s >= (shi[..., a] - base).astype(np.float32).astype(np.float64)
    return bool(ok[occ].all())


def soup(n, seed=7):
    """n triangles: centres uniform in [-10, 10]^3, vertices at centre + N(0, 0.3); TRI_DT"""
    rs = np.random.RandomState(seed)
    c = rs.uniform(-10, 10, size=(n, 1, 3))
    t = np.zeros(n, dtype=O.TRI_DT)
    t["p"] = (c + rs.normal(0, 0.3, size=(n, 3, 3))).astype(np.float32)
    e0, e1 = t["p"][:, 1] - t["p"][:, 0], t["p"][:, 2] - t["p"][:, 0]
    nrm = np.cross(e0, e1)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-20)
    t["n"] = nrm[:, None, :].astype(np.float32)
    t["matid"] = 0
    return t


def soup_material():
    """diffuse and a little emissive: every hit shows in an image"""
    m = np.zeros(1, dtype=O.MAT_DT)
    m["dtex"], m["etex"], m["stex"] = -1, -1, -1
    m["kd"], m["ke"], m["illum"], m["dissolve"], m["ior"] = (0.7, 0.6, 0.5), (0.5, 0.4, 0.3), 2, 1.0, 1.5
    return m


def wave(triangles):
    """y += 1.5 sin(0.7 x) + 0.8 cos(0.9 z); x *= 1.1 (from the rest pose's x and z)"""
    t = np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1).copy()
    p = t["p"].astype(np.float64)
    p[..., 1] += 1.5 * np.sin(0.7 * p[..., 0]) + 0.8 * np.cos(0.9 * p[..., 2])
    p[..., 0] *= 1.1
    t["p"] = p.astype(np.float32)
    return t


def jitter(triangles, seed=11):
    t = np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1).copy()
    t["p"] = (t["p"].astype(np.float64) + np.random.RandomState(seed).normal(0, 0.2, size=t["p"].shape)).astype(np.float32)
    return t


def rays_in_box(triangles, n, seed=3):
    """origins uniform in the scene's box, tmin 1e-4, directions N(0, 1)"""
    rs = np.random.RandomState(seed)
    p = np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1)["p"].reshape(-1, 3)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = rs.uniform(p.min(0), p.max(0), size=(n, 3))
    rays[:, 3] = 1e-4
    rays[:, 4:7] = rs.normal(size=(n, 3))
    return rays
