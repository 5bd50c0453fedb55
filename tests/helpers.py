"""Shared helpers of the test-suite: load fixtures into oracle / product objects."""
import os

import numpy as np

from oracle import oracle_py as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden_scene(name):
    """(cfg, tri_indices, nodes, tris, mats, woop) produced by the REFERENCE code for fixture `name`."""
    cfg, idx, nodes = O.load_bvh_file(os.path.join(GOLDEN, name + ".bvh"))
    tris = np.fromfile(os.path.join(GOLDEN, name + ".tris"), dtype=O.TRI_DT)
    mats = np.fromfile(os.path.join(GOLDEN, name + ".mats"), dtype=O.MAT_DT)
    woop = np.fromfile(os.path.join(GOLDEN, name + ".woop"), dtype=np.float32).reshape(-1, 12)
    return cfg, idx, nodes, tris, mats, woop


def oracle_scene_from_golden(name):
    _, idx, nodes, tris, mats, woop = golden_scene(name)
    return O.Scene(nodes, idx, tris, mats, woop=woop)


def oracle_scene_from_instance(inst):
    return O.Scene(inst.bvh.nodes, inst.bvh.tri_indices, inst.scene.triangles, inst.scene.materials, textures=inst.scene.textures)


def oracle_params_from_config(c):
    ip, iv = O.camera(c.fov, c.yaw, c.pitch, c.width, c.height)
    return O.make_params(c.width, c.height, list(c.position), ip, iv, stack_size=c.stack_size, max_bounce=c.max_bounce,
                         subpixel=c.subpixel, tmp_life=c.tmp_lifetime, tmin=c.ray_tmin, clamp=c.clamp, sun=list(c.sun))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_rays(tris_bytes, n, seed):
    rs = np.random.RandomState(seed)
    p = np.frombuffer(np.ascontiguousarray(tris_bytes).tobytes(), dtype=O.TRI_DT)["p"].reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = rs.uniform(lo, hi, size=(n, 3))
    rays[:, 3] = 1e-4
    rays[:, 4:7] = rs.normal(size=(n, 3))
    k = max(1, n // 20)
    rays[:k, 4] = 0
    rays[k:2 * k, 5] = 0
    rays[2 * k:3 * k, 4:6] = 0
    rays[3 * k:4 * k, 4:7] *= 1e-30
    return rays


def cpu_scene(cache, name, **kw):
    """(api.Scene, api.WideBVH, O.Scene) of a generated scene, built on the host only (no GPU needed)."""
    from adypt_amd import api, scenes
    spec = scenes.make_scene(name, cache, width=64, height=36, **kw)
    cfg = api.InstanceConfig()
    assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
    sc = api.Scene()
    assert sc.LoadFromFile(cfg.m_obj_filename)
    b = api.WideBVH()
    if not b.LoadFromFile(cfg.m_bvh_filename, cfg.bvh_params()):
        b.Build(sc, cfg.bvh_params())
        b.SaveToFile(cfg.m_bvh_filename, cfg.bvh_params())
    return sc, b, O.Scene(b.nodes, b.tri_indices, sc.triangles, sc.materials)


# tmin classes of mixed_rays, ray i in class i % N_TMIN_CLASSES; the last three are the hit's own t and its float neighbours
TMIN_CLASSES = ("zero", "1e-4", "uniform", "beyond", "negative", "at_hit", "above_hit", "below_hit")
N_TMIN_CLASSES = len(TMIN_CLASSES)
# direction classes, ray i in class (i // N_TMIN_CLASSES) % N_DIR_CLASSES: every 48 consecutive rays hold every pair of classes
DIR_CLASSES = ("plain", "minus_zero", "ooeps", "ooeps_ulp", "denormal", "all_tiny")
N_DIR_CLASSES = len(DIR_CLASSES)
OOEPS = np.float32(2.0 ** -64)  # traversal.glsl:16


def tmin_class(n):
    return np.arange(n) % N_TMIN_CLASSES


def scene_diag(tris_bytes):
    p = np.frombuffer(np.ascontiguousarray(tris_bytes).tobytes(), dtype=O.TRI_DT)["p"].reshape(-1, 3).astype(np.float64)
    return float(np.linalg.norm(p.max(0) - p.min(0)))


def mixed_rays(tris_bytes, n, seed, closest):
    """(n, 8) rays whose tmin and direction vary within every wave (random_rays keeps tmin = 1e-4).  tmin by class (TMIN_CLASSES):
    0, 1e-4, uniform in [0, diag / 2], 2 diag (beyond the scene: every ray misses), -diag / 2 (hits behind the origin count), and
    exactly the binary32 t of the ray's own closest hit at tmin 1e-4 and the floats just above and below it — the boundary of the
    strict `t > tmin` (traversal.glsl:235).  closest(rays) -> HIT_DT records gives that t (the oracle's first pass).
    Directions by class (DIR_CLASSES): components of -0.0, exactly +-2^-64, one ulp either side of +-2^-64, denormals, and all
    three tiny with mixed signs — the values around the substitution of traversal.glsl:16-19."""
    rs = np.random.RandomState(seed)
    p = np.frombuffer(np.ascontiguousarray(tris_bytes).tobytes(), dtype=O.TRI_DT)["p"].reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    diag = scene_diag(tris_bytes)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = rs.uniform(lo, hi, size=(n, 3))
    d = rs.normal(size=(n, 3)).astype(np.float32)
    dcls = (np.arange(n) // N_TMIN_CLASSES) % N_DIR_CLASSES
    sign = np.where(rs.uniform(size=(n, 3)) < 0.5, np.float32(-1), np.float32(1))
    comp = rs.randint(0, 3, size=n)
    two = rs.uniform(size=n) < 0.3  # a second component of the same kind
    comp2 = (comp + 1 + rs.randint(0, 2, size=n)) % 3
    below, above = np.nextafter(OOEPS, np.float32(0)), np.nextafter(OOEPS, np.float32(1))
    denorm = (rs.randint(1, 1 << 23, size=(n, 3)).astype(np.uint32)).view(np.float32)
    tiny_menu = np.array([0.0, OOEPS, below, above, np.float32(1e-30), np.float32(3e-20), np.float32(2.0 ** -63)], np.float32)
    for i in range(n):
        c, cs = dcls[i], [comp[i], comp2[i]] if two[i] else [comp[i]]
        for k in cs:
            if c == 1:
                d[i, k] = -0.0
            elif c == 2:
                d[i, k] = sign[i, k] * OOEPS
            elif c == 3:
                d[i, k] = sign[i, k] * (below if (i // 48) % 2 else above)
            elif c == 4:
                d[i, k] = sign[i, k] * denorm[i, k]
        if c == 5:
            pick = tiny_menu[rs.randint(0, len(tiny_menu), size=3)]
            pick[rs.randint(0, 3)] = np.float32(1e-30)  # at least one component below 2^-64
            d[i] = sign[i] * pick
            if pick[0] == 0.0 and rs.uniform() < 0.5:
                d[i, 0] = -0.0
    rays[:, 4:7] = d
    tc = tmin_class(n)
    rays[:, 3] = 1e-4
    first = closest(rays)["t"]
    t_of = {0: np.float32(0.0), 1: np.float32(1e-4), 3: np.float32(2 * diag), 4: np.float32(-0.5 * diag)}
    for k, v in t_of.items():
        rays[tc == k, 3] = v
    rays[tc == 2, 3] = rs.uniform(0, 0.5 * diag, size=int((tc == 2).sum())).astype(np.float32)
    rays[tc == 5, 3] = first[tc == 5]
    rays[tc == 6, 3] = np.nextafter(first[tc == 6], np.float32(np.inf))
    rays[tc == 7, 3] = np.nextafter(first[tc == 7], np.float32(-np.inf))
    return rays


def check_against_fp64_truth(tris, rays, hits, any_hit=False, eps=2e-6, tol_t=1e-5):
    """Holds traversal records (HIT_DT: the oracle's or the kernel's) against the binary64 truth (O.brute_force_ex).  A ray passes
    when its triangle is the truth's (at the same t); or both hit at the same t (a tie); or — the only excused disagreement — the
    deciding hit lies within eps of a triangle edge or within tol_t of tmin, where binary32 and binary64 may legitimately decide
    differently.  Any other disagreement fails, a farther hit or a missed one included.  eps and tol_t are fractions of the scene's
    diagonal: the binary32 Woop test errs in scene units (measured: t by up to 5e-6, edges by up to 3e-7 of the diagonal).
    any_hit: the verdict (hit or not) must be the truth's unless every true hit is within those bounds, and the triangle reported
    must be hit by the ray in binary64 at the reported t (or lie within the bounds).  Returns the mask of excused rays."""
    diag = scene_diag(tris)
    eps, tol_t = eps * diag, tol_t * diag
    tmin = rays[:, 3].astype(np.float64)
    ti, tr = O.brute_force_ex(tris, rays, "any" if any_hit else "closest")
    gid = hits["tri_id"]
    _, gr = O.brute_force_ex(tris, rays, "given", gid)
    g_hit, t_hit = gid >= 0, ti >= 0
    t32 = hits["t"].astype(np.float64)
    assert (np.abs(t32 - gr[:, 0])[g_hit] <= tol_t).all(), "a hit's t is not its triangle's binary64 t"
    # the kernel's triangle in binary64: inside, or within the bounds of the edges and of tmin
    g_out = g_hit & ((gr[:, 3] < -eps) | (gr[:, 0] - tmin < -tol_t))
    assert not g_out.any(), "hits the ray does not have in binary64: rays %s" % np.nonzero(g_out)[0][:10]
    g_marginal = g_hit & ((gr[:, 3] <= eps) | (gr[:, 0] - tmin <= tol_t))
    t_marginal = t_hit & ((tr[:, 3] <= eps) | (tr[:, 0] - tmin <= tol_t))  # the truth's deciding hit
    if any_hit:
        bad = ~g_hit & t_hit & ~t_marginal
        assert not bad.any(), "any-hit missed a clear hit: rays %s" % np.nonzero(bad)[0][:10]
        excused = (g_hit & ~t_hit) | (~g_hit & t_hit)
        assert not (excused & ~(g_marginal | t_marginal)).any()
        return excused
    same = gid == ti
    tie = g_hit & t_hit & ~same & (np.abs(gr[:, 0] - tr[:, 0]) <= tol_t)
    nearer = g_hit & ~same & ~tie & (~t_hit | (gr[:, 0] < tr[:, 0]))   # the kernel took a hit the truth rejects: must be marginal
    farther = t_hit & ~same & ~tie & ~nearer                            # the kernel passed the truth's hit: it must be marginal
    bad = (nearer & ~g_marginal) | (farther & ~t_marginal)
    assert not bad.any(), "disagreement with the fp64 truth: rays %s (kernel %s, truth %s)" % (
        np.nonzero(bad)[0][:10], gid[bad][:10], ti[bad][:10])
    return nearer | farther
