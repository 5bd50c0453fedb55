"""CPU tests of the UNPINNED half of the oracle (oracle/oracle.cpp: traversal + Render).  The reference has no tests or
fixtures for its shaders and the GLSL cannot run here, so these are the strongest substitutes available:

  * the shading pieces — reflect / refract / Fresnel (shaders/pathtracer.glsl:160-196), AlignDirection (:66-71),
    SampleHemisphere (:52-64) — against independent binary64 evaluations and textbook identities;
  * closed scenes whose radiance is known exactly (black furnace = 0, emissive furnace = a geometric series);
  * a whole image against an INDEPENDENT path tracer written here in numpy/binary64 straight from the GLSL, with brute-force
    Möller–Trumbore intersection instead of the CWBVH traversal + Woop test, and libm sin / cos / pow instead of the canonical
    series.  Same sample sequence, different everything else: the images must agree except where a discrete decision flips.

Nothing here makes the parity "pinned" — there is no reference output to pin it to — but a shared misreading of the GLSL now has to
survive two writings by different routes."""
import os

import numpy as np
import pytest

from oracle import oracle_py as O
from tests.helpers import GOLDEN, golden_scene

F64 = np.float64


def unit(v):
    v = np.asarray(v, F64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_units(rs, n):
    return unit(rs.normal(size=(n, 3))).astype(np.float32)


def mats(n, illum, kd=(0.5, 0.5, 0.5), ks=(0.5, 0.5, 0.5), shininess=1.0, ior=1.5):
    m = np.zeros(n, dtype=O.MAT_DT)
    m["dtex"] = m["etex"] = m["stex"] = -1
    m["kd"], m["ks"], m["illum"], m["shininess"], m["ior"], m["dissolve"] = kd, ks, illum, shininess, ior, 1.0
    return m


# ------------------------------------------------------------------------------------------------------------------
# reflect / refract / Fresnel
# ------------------------------------------------------------------------------------------------------------------
def test_mirror_reflection_closed_form():
    rs = np.random.RandomState(1)
    n = 20000
    nrm, d = random_units(rs, n), random_units(rs, n)
    out = O.scatter(mats(n, 3, ks=(0.9, 0.8, 0.7)), nrm, d, rs.uniform(size=(n, 2)))
    N, D = nrm.astype(F64), d.astype(F64)
    N = np.where((np.sum(D * N, -1) > 0)[:, None], -N, N)            # illum < 6: the normal faces the ray (pathtracer.glsl:141-142)
    want = D - 2.0 * np.sum(N * D, -1, keepdims=True) * N             # reflect(I, N) = I - 2 dot(N, I) N
    assert np.abs(out[:, :3] - want).max() < 2e-6
    assert np.allclose(np.linalg.norm(out[:, :3].astype(F64), axis=1), 1.0, atol=2e-6)
    assert np.allclose(np.sum(out[:, :3] * N, -1), -np.sum(D * N, -1), atol=2e-6)  # angle out = angle in
    assert np.array_equal(out[:, 3:6], np.broadcast_to(np.float32([0.9, 0.8, 0.7]), (n, 3))) and (out[:, 7] == 1).all()


def test_dielectric_fresnel_and_directions_against_fp64():
    rs = np.random.RandomState(2)
    n = 40000
    nrm, d = random_units(rs, n), random_units(rs, n)
    ior = rs.choice([1.0, 1.33, 1.5, 2.4], size=n).astype(np.float32)
    r = rs.uniform(size=(n, 2)).astype(np.float32)
    m = mats(n, 7)
    m["ior"] = ior
    m["illum"][::2] = 6
    out = O.scatter(m, nrm, d, r)
    N, D, eta0 = nrm.astype(F64), d.astype(F64), ior.astype(F64)
    cosi = np.sum(D * N, -1)
    exiting = cosi > 0                                                 # travelling along the normal = leaving the medium
    etai, etat = np.where(exiting, eta0, 1.0), np.where(exiting, 1.0, eta0)
    Np = np.where(exiting[:, None], N, -N)                             # the shader's normal after its flip: along the ray
    ci = np.abs(cosi)
    # textbook Fresnel reflectance of unpolarised light from the angles (independent of the shader's Rs / Rp naming)
    sini = np.sqrt(np.maximum(0.0, 1.0 - ci * ci))
    sint = etai / etat * sini
    tir = sint >= 1.0
    cost = np.sqrt(np.maximum(0.0, 1.0 - np.minimum(sint, 1.0) ** 2))
    r_s = (etai * ci - etat * cost) / (etai * ci + etat * cost)
    r_p = (etat * ci - etai * cost) / (etat * ci + etai * cost)
    F = np.where(tir, 1.0, 0.5 * (r_s ** 2 + r_p ** 2))
    # binary32 cancellation makes the formula as written ill-conditioned at grazing incidence (cos -> 0) and at the critical
    # angle (sin_t -> 1): compare where it is well conditioned, require a valid reflectance everywhere
    conditioned = (ci > 0.02) & (np.abs(1.0 - sint) > 0.02)
    assert conditioned.mean() > 0.9
    assert np.abs(out[:, 6] - F)[conditioned].max() < 5e-6
    assert ((out[:, 6] >= 0) & (out[:, 6] <= 1.0 + 1e-6)).all()
    # normal incidence: ((n - 1) / (n + 1))^2
    head = O.scatter(mats(1, 7, ior=1.5), [[0, 0, 1]], [[0, 0, -1]], [[0.9, 0.0]])
    assert abs(head[0, 6] - 0.04) < 1e-6
    # the decision and the directions, exactly as the shader writes them (pathtracer.glsl:188-196), in binary64
    eta = etai / etat
    cos2 = 1.0 - eta * eta * (1.0 - ci * ci)
    refr = (cos2 > 0) & (r[:, 0].astype(F64) >= F)
    clear = conditioned & (np.abs(r[:, 0] - F) > 1e-5) & (np.abs(cos2) > 1e-4)   # away from the decision boundaries
    t = unit(D * eta[:, None] + Np * (eta * ci + np.sqrt(np.maximum(cos2, 0.0)))[:, None])
    refl = D - 2.0 * np.sum(Np * D, -1, keepdims=True) * Np
    want = np.where(refr[:, None], t, refl)
    err = np.abs(out[:, :3] - want).max(axis=1)
    assert err[clear].max() < 5e-6
    assert (np.abs(out[:, 3:6] - 1.0) == 0).all() and (out[:, 7] == 1).all()    # throughput untouched, never terminates
    assert tir.sum() > 100 and refr.sum() > 1000 and (~refr).sum() > 1000           # every branch exercised
    assert not refr[tir].any()                                                      # total internal reflection always reflects


def test_other_illum_values_pass_straight_through():
    rs = np.random.RandomState(3)
    n = 64
    nrm, d = random_units(rs, n), random_units(rs, n)
    for illum in (0, 8, 9, 11, -3):
        out = O.scatter(mats(n, illum), nrm, d, rs.uniform(size=(n, 2)))
        assert np.array_equal(out[:, :3], d) and (out[:, 3:6] == 1).all() and (out[:, 7] == 1).all()


def test_diffuse_and_glossy_lobes():
    rs = np.random.RandomState(4)
    n = 30000
    nrm, d = random_units(rs, n), random_units(rs, n)
    r = rs.uniform(size=(n, 2)).astype(np.float32)
    N = np.where((np.sum(d.astype(F64) * nrm, -1) > 0)[:, None], -nrm.astype(F64), nrm.astype(F64))
    # illum 1, and illum 2 with Ns * 0.01 <= 0.3 (falls through to the diffuse case, pathtracer.glsl:144-158)
    for m in (mats(n, 1, kd=(0.2, 0.4, 0.6)), mats(n, 2, kd=(0.2, 0.4, 0.6), shininess=30.0)):
        out = O.scatter(m, nrm, d, r)
        assert (out[:, 7] == 1).all() and np.array_equal(out[:, 3:6], np.broadcast_to(np.float32([0.2, 0.4, 0.6]), (n, 3)))
        assert (np.sum(out[:, :3] * N, -1) > -1e-6).all()                  # in the hemisphere of the facing normal
        assert np.allclose(np.linalg.norm(out[:, :3].astype(F64), axis=1), 1.0, atol=3e-6)
        assert np.array_equal(out[:, :3], O.align_direction(O.sample_hemisphere(r, 0.0), N.astype(np.float32)))
    # illum 2 with e = Ns * 0.01 > 0.3: lobe about the mirror direction, weight Kd + Ks * cos^e, dead below the surface
    e = 2.0
    m = mats(n, 2, kd=(0.3, 0.3, 0.1), ks=(0.5, 0.4, 0.3), shininess=200.0)
    out = O.scatter(m, nrm, d, r)
    D = d.astype(F64)
    R = D - 2.0 * np.sum(N * D, -1, keepdims=True) * N
    new = out[:, :3].astype(F64)
    alive = out[:, 7] == 1
    assert np.array_equal(alive, np.sum(out[:, :3] * N.astype(np.float32), -1, dtype=np.float32) >= 0) or (alive == (np.sum(new * N, -1) >= -1e-7)).all()
    w = np.float64([0.3, 0.3, 0.1]) + np.float64([0.5, 0.4, 0.3]) * (np.sum(new * R, -1) ** e)[:, None]
    assert np.abs(out[alive, 3:6] - w[alive]).max() < 1e-5
    assert (out[~alive, 3:6] == 1).all()                                       # `return ret` happens before the throughput update
    assert 0.02 < (~alive).mean() < 0.6


# ------------------------------------------------------------------------------------------------------------------
# AlignDirection / SampleHemisphere
# ------------------------------------------------------------------------------------------------------------------
def test_align_direction_builds_an_orthonormal_frame():
    rs = np.random.RandomState(5)
    n = 20000
    t = random_units(rs, n)
    t[:200, 0] = 0.0                                                        # |target.x| <= 0.01 takes the other helper axis
    t[:200] = unit(t[:200] + [0, 1e-3, 0]).astype(np.float32)
    ex = O.align_direction(np.tile(np.float32([1, 0, 0]), (n, 1)), t).astype(F64)
    ey = O.align_direction(np.tile(np.float32([0, 1, 0]), (n, 1)), t).astype(F64)
    ez = O.align_direction(np.tile(np.float32([0, 0, 1]), (n, 1)), t).astype(F64)
    T = t.astype(F64)
    assert np.array_equal(ez.astype(np.float32), t)                         # dir.z * target with dir = (0, 0, 1), fma of exact zeros
    for a, b in ((ex, ey), (ex, T), (ey, T)):
        assert np.abs(np.sum(a * b, -1)).max() < 3e-6
    for a in (ex, ey):
        assert np.abs(np.linalg.norm(a, axis=1) - 1).max() < 3e-6
    assert np.abs(np.cross(T, ex) - ey).max() < 3e-6                        # v = cross(target, u): right-handed
    d = random_units(rs, n)
    out = O.align_direction(d, t).astype(F64)
    want = d[:, :1] * ex + d[:, 1:2] * ey + d[:, 2:3] * T
    assert np.abs(out - want).max() < 3e-6
    assert np.abs(np.sum(out * T, -1) - d[:, 2]).max() < 3e-6               # the polar angle about the target is preserved


@pytest.mark.parametrize("e", [0.0, 0.5, 2.0, 25.0, 400.0])
def test_sample_hemisphere_moments(e):
    k = 384
    g = (np.arange(k) + 0.5) / k                                             # stratified (r.x, r.y) grid
    r = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    d = O.sample_hemisphere(r, e).astype(F64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 3e-6 and (d[:, 2] >= 0).all()
    # cos(theta) = (1 - r.y)^(1 / (e + 1))  =>  E[cos] = (e + 1) / (e + 2), E[cos^2] = (e + 1) / (e + 3); phi uniform
    assert abs(d[:, 2].mean() - (e + 1) / (e + 2)) < 2e-4
    assert abs((d[:, 2] ** 2).mean() - (e + 1) / (e + 3)) < 2e-4
    assert abs(d[:, 0].mean()) < 1e-6 and abs(d[:, 1].mean()) < 1e-6
    assert abs((d[:, 0] ** 2).mean() - (d[:, 1] ** 2).mean()) < 1e-6
    # against the same formula in binary64 with libm
    phi = r[:, 0].astype(np.float32) * np.float32(6.28318530718)
    ct = (1.0 - r[:, 1].astype(F64)) ** (1.0 / (np.float64(np.float32(e)) + 1.0))
    st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
    want = unit(np.stack([st * np.cos(phi.astype(F64)), st * np.sin(phi.astype(F64)), ct], -1))
    assert np.abs(d - want).max() < (2e-6 if e < 100 else 5e-5)             # sin(theta) = sqrt(1 - cos^2) amplifies rounding near the pole


# ------------------------------------------------------------------------------------------------------------------
# furnace scenes: radiance known in closed form
# ------------------------------------------------------------------------------------------------------------------
def _box_scene(tmp_path, kd, ke, name):
    """Unit-ish closed box around the origin, 12 triangles, one diffuse material; built by the product's host loader and
    SBVH -> CWBVH8 builder (CPU code, needs no GPU), handed to the oracle as arrays."""
    from adypt_amd import api
    v = [(x, y, z) for x in (-2, 2) for y in (-1.5, 1.5) for z in (-2.5, 2.5)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    obj = ["mtllib %s.mtl" % name] + ["v %g %g %g" % p for p in v] + ["usemtl wall"]
    for a, b, c, d in quads:
        obj += ["f %d %d %d" % (a + 1, b + 1, c + 1), "f %d %d %d" % (a + 1, c + 1, d + 1)]
    (tmp_path / (name + ".obj")).write_text("\n".join(obj) + "\n")
    (tmp_path / (name + ".mtl")).write_text("newmtl wall\nKd %g %g %g\nKs 0 0 0\nKe %g %g %g\nNs 1\nNi 1\nd 1\nillum 1\n" % (tuple(kd) + tuple(ke)))
    sc = api.Scene()
    assert sc.LoadFromFile(str(tmp_path / (name + ".obj")))
    b = api.WideBVH()
    b.Build(sc, api.InstanceConfig().bvh_params())
    return O.Scene(b.nodes, b.tri_indices, sc.triangles, sc.materials)


def _render_box(scene, sobol_matrices, bounces, spp, sun=(0.0, 0.0, 0.0), clamp=1e6, tmin=1e-4):
    w, h = 48, 32
    ip, iv = O.camera(70.0, 30.0, -10.0, w, h)
    P = O.make_params(w, h, [0.3, -0.2, 0.4], ip, iv, stack_size=16, max_bounce=bounces, subpixel=2, tmp_life=3, tmin=tmin, clamp=clamp, sun=list(sun))
    st = O.PathTracerState(w, h)
    stats = O.pt_frames(scene, P, O.shift_bytes(9, w, h), sobol_matrices, st, spp).as_dict()
    return st.accum[..., :3], stats


def test_black_furnace_is_exactly_black(tmp_path, sobol_matrices):
    box = _box_scene(tmp_path, (0.8, 0.7, 0.6), (0, 0, 0), "black")
    img, st = _render_box(box, sobol_matrices, 6, 5)
    assert not img.any() and st["rays"] > 40000                  # closed box, no emitter, no sun: nothing to pick up
    # With the sun on, only a path that LEAVES the closed box picks anything up.  The reference's intersection is not
    # watertight: a path vertex closer than rayTMin to the next wall steps through it (traversal.glsl: t > tmin), the fp32 Woop
    # test can miss along shared edges, and the Sobol point of frame 0 is 0.5 in every dimension, so a path repeats the same local
    # direction at every bounce and drifts into the corners.  Leaks are rare, never negative light, and bounded by the sun term.
    img, st = _render_box(box, sobol_matrices, 6, 5, sun=(12, 11, 10), clamp=4.0)
    assert 1.0 - st["hits"] / st["rays"] < 0.02 and (img.sum(-1) > 0).mean() < 0.25
    assert img.min() >= 0 and img.max() <= 4.0


@pytest.mark.parametrize("bounces", [1, 3, 8])
def test_emissive_furnace_is_a_geometric_series(bounces, tmp_path, sobol_matrices):
    rho, E = np.float32([0.5, 0.25, 0.8]), np.float32([1.0, 2.0, 0.5])
    img, st = _render_box(_box_scene(tmp_path, rho, E, "lit%d" % bounces), sobol_matrices, bounces, 4)
    # Render: ret += color * Ke at every hit, color *= Kd (uniform hemisphere, no cosine, no 1/pi: pathtracer.glsl:139,154-157);
    # every bounce of every path hits a wall, so each sample = E * (1 + rho + ... + rho^(B-1)), accumulated in this fp32 order
    want, color = np.zeros(3, np.float32), np.ones(3, np.float32)
    for _ in range(bounces):
        want = (color.astype(F64) * E + want).astype(np.float32)  # fma(color, Ke, ret): one rounding
        color = color * rho
    exact = E.astype(F64) * (1 - rho.astype(F64) ** bounces) / (1 - rho.astype(F64))
    assert np.allclose(want, exact, rtol=1e-6)
    # the running mean of identical samples: (x * k + x) / (k + 1) may differ from x by an ulp per frame.  A path that leaks
    # out of the box (see the black furnace) loses the rest of its series: never brighter, and rare
    assert (img / want < 1 + 4e-7).all()
    assert (np.abs(img / want - 1).max(axis=-1) < 4e-7).mean() > (0.999 if bounces < 3 else 0.85)


# ------------------------------------------------------------------------------------------------------------------
# a whole image against an independent binary64 brute-force path tracer
# ------------------------------------------------------------------------------------------------------------------
def _independent_path_tracer(tris, mats_, w, h, cam, origin, tmin, bounces, subpixel, clamp, sun, shift, sobol_pts, spp_count):
    """shaders/pathtracer.glsl:101-227 in numpy / binary64, tmpLifetime = 1 (every frame traces its primary rays).  Brute-force
    Möller–Trumbore over all triangles; hit barycentrics in the shader's convention (position = p1*u + p2*v + p3*(1-u-v))."""
    P = tris["p"].astype(F64)
    Nn = tris["n"].astype(F64)
    v2, e1, e2 = P[:, 2], P[:, 0] - P[:, 2], P[:, 1] - P[:, 2]
    matid = tris["matid"]
    ip = np.asarray(cam[0], F64).reshape(4, 4).T  # column-major -> M[row, col]
    iv = np.asarray(cam[1], F64).reshape(4, 4).T
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.reshape(-1).astype(F64), ys.reshape(-1).astype(F64)
    npx = w * h
    sh = shift.reshape(-1, 2).astype(F64) / 255.0
    accum = np.zeros((npx, 3), F64)

    def intersect(o, d, alive):
        dn = unit(d)
        best_t = np.full(len(o), 1e9)
        best = np.full(len(o), -1)
        bu, bv = np.zeros(len(o)), np.zeros(len(o))
        idx = np.nonzero(alive)[0]
        for k in range(len(P)):
            pv = np.cross(dn[idx], e2[k])
            det = pv @ e1[k]
            ok = det != 0
            inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
            tv = o[idx] - v2[k]
            u = np.sum(tv * pv, -1) * inv
            qv = np.cross(tv, e1[k])
            v = np.sum(dn[idx] * qv, -1) * inv
            t = (qv @ e2[k]) * inv
            hit = ok & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > tmin) & (t < best_t[idx])
            sel = idx[hit]
            best_t[sel], best[sel], bu[sel], bv[sel] = t[hit], k, u[hit], v[hit]
        return best, bu, bv

    def sobol(frame, b):
        p = sobol_pts[frame, 2 * b:2 * b + 2].astype(F64) + sh
        return p - np.floor(p)

    def hemisphere(r, e):
        phi = r[:, 0] * 6.28318530718
        ct = (1.0 - r[:, 1]) ** (1.0 / (e + 1.0))
        st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
        return unit(np.stack([st * np.cos(phi), st * np.sin(phi), ct], -1))

    def align(d, t):
        a = np.where((np.abs(t[:, 0]) > 0.01)[:, None], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0])
        u = unit(np.cross(a, t))
        v = np.cross(t, u)
        return d[:, :1] * u + d[:, 1:2] * v + d[:, 2:3] * t

    for spp in range(spp_count):
        si = spp % (subpixel * subpixel)
        bias = np.array([(si // subpixel) / subpixel, (si % subpixel) / subpixel])
        scr = np.stack([2.0 * (xs + bias[0]) / w - 1.0, -(2.0 * (ys + bias[1]) / h - 1.0), np.ones(npx), np.ones(npx)], -1)
        d = unit((scr @ ip.T)[:, :3] @ iv[:3, :3].T)
        o = np.tile(np.asarray(origin, F64), (npx, 1))
        ret, color = np.zeros((npx, 3)), np.ones((npx, 3))
        alive = np.ones(npx, bool)
        for b in range(bounces):
            tri, u, v = intersect(o, d, alive)
            miss = alive & (tri < 0)
            ret[miss] += color[miss] * sun
            alive &= tri >= 0
            if not alive.any():
                break
            i = np.nonzero(alive)[0]
            k = tri[i]
            uu, vv = u[i][:, None], v[i][:, None]
            ww = 1.0 - uu - vv
            normal = unit(Nn[k, 0] * uu + Nn[k, 1] * vv + Nn[k, 2] * ww)
            o[i] = P[k, 0] * uu + P[k, 1] * vv + P[k, 2] * ww
            m = mats_[matid[k]]
            ret[i] += color[i] * m["ke"]
            di = d[i]
            illum = m["illum"].copy()
            flip = (illum < 6) & (np.sum(di * normal, -1) > 0)
            normal[flip] = -normal[flip]
            r = sobol(spp, b)[i]
            e = m["shininess"].astype(F64) * 0.01
            glossy = (illum == 2) & (e > 0.3)
            diffuse = (illum == 1) | ((illum == 2) & ~glossy)
            mirror = (illum >= 3) & (illum <= 5)
            glass = (illum == 6) | (illum == 7)
            nd, nc, dead = di.copy(), color[i].copy(), np.zeros(len(i), bool)
            refl = di - 2.0 * np.sum(normal * di, -1, keepdims=True) * normal
            if glossy.any():
                g = glossy
                s = np.empty((g.sum(), 3))
                for ev in np.unique(e[g]):
                    sel = e[g] == ev
                    s[sel] = hemisphere(r[g][sel], ev)
                nd[g] = align(s, refl[g])
                below = np.sum(nd[g] * normal[g], -1) < 0
                dead[np.nonzero(g)[0][below]] = True
                nc[g] = nc[g] * (m["kd"][g] + m["ks"][g] * (np.sum(nd[g] * refl[g], -1) ** e[g])[:, None])
            if diffuse.any():
                nd[diffuse] = align(hemisphere(r[diffuse], 0.0), normal[diffuse])
                nc[diffuse] = nc[diffuse] * m["kd"][diffuse]
            if mirror.any():
                nd[mirror] = refl[mirror]
                nc[mirror] = nc[mirror] * m["ks"][mirror]
            if glass.any():
                g = glass
                n_, d_, eta0 = normal[g], di[g], m["ior"][g].astype(F64)
                cosi = np.sum(d_ * n_, -1)
                out_ = cosi > 0
                etai, etat = np.where(out_, eta0, 1.0), np.where(out_, 1.0, eta0)
                n_ = np.where(out_[:, None], n_, -n_)
                cosi = np.abs(cosi)
                eta = etai / etat
                sint = eta * np.sqrt(np.maximum(0.0, 1.0 - cosi * cosi))
                cost = np.sqrt(np.maximum(0.0, 1.0 - np.minimum(sint, 1.0) ** 2))
                Rs = (etat * cosi - etai * cost) / (etat * cosi + etai * cost)
                Rp = (etai * cosi - etat * cost) / (etai * cosi + etat * cost)
                Fr = np.where(sint >= 1.0, 1.0, 0.5 * (Rs * Rs + Rp * Rp))
                cos2 = 1.0 - eta * eta * (1.0 - cosi * cosi)
                refract = (cos2 > 0) & (r[g][:, 0] >= Fr)
                t = unit(d_ * eta[:, None] + n_ * (eta * cosi + np.sqrt(np.maximum(cos2, 0.0)))[:, None])
                rf = d_ - 2.0 * np.sum(n_ * d_, -1, keepdims=True) * n_
                nd[g] = np.where(refract[:, None], t, rf)
            d[i], color[i] = nd, nc
            alive[i[dead]] = False
        r = np.minimum(ret, clamp)
        accum = (accum * spp + r) / (spp + 1)
    return accum.reshape(h, w, 3)


@pytest.mark.parametrize("tmin,bounces", [(1e-4, 5), (0.05, 5), (0.0, 1)])
def test_image_against_independent_fp64_brute_force_path_tracer(sobol_matrices, tmin, bounces):
    """tmin 1e-4 is every scene's; 0.05 skips the geometry just past every bounce point.  At tmin 0 a bounce's ray finds the surface it
    leaves again whenever binary32 puts its hit at t > 0 (what a positive tmin is for) and binary64 does not, so the two tracers
    part after the first bounce: that case traces the camera's rays only."""
    _, idx, nodes, tris, mats_, woop = golden_scene("tiny0")
    from adypt_amd import scenes
    cam = scenes._SCENE_TABLE["tiny0"][3]
    w, h, spp, subpixel, clamp, sun = 48, 27, 6, 2, 4.0, np.float64([12.0, 11.0, 10.0])
    ip, iv = O.camera(cam["fov"], cam["yaw"], cam["pitch"], w, h)
    P = O.make_params(w, h, list(cam["position"]), ip, iv, stack_size=24, max_bounce=bounces, subpixel=subpixel, tmp_life=1, tmin=tmin, clamp=clamp, sun=list(sun))
    st = O.PathTracerState(w, h)
    shift = O.shift_bytes(4242, w, h)
    O.pt_frames(O.Scene(nodes, idx, tris, mats_, woop=woop), P, shift, sobol_matrices, st, spp)
    pts = O.sobol(sobol_matrices, 2 * bounces, 0, spp).reshape(spp, 2 * bounces)
    mine = _independent_path_tracer(tris, mats_, w, h, (ip, iv), cam["position"], tmin, bounces, subpixel, clamp, sun, shift, pts, spp)
    orc = st.accum[..., :3].astype(F64)
    assert orc.mean() > 0.05
    diff = np.abs(orc - mine).max(axis=-1)
    # same samples, independent intersection + arithmetic: pixels agree to rounding unless a discrete decision (edge hit,
    # Fresnel coin, glossy sample at the horizon) flips for one of the samples
    assert (diff < 1e-4).mean() > 0.97, "only %.3f of the pixels agree" % (diff < 1e-4).mean()
    assert abs(orc.mean() - mine.mean()) < 3e-3 * orc.mean()
    # every material class is in view and contributes
    hit_mats = set()
    prim = O.primary_frame(O.Scene(nodes, idx, tris, mats_, woop=woop), P, 0)[1]
    for t in np.unique(prim["tri_id"][prim["tri_id"] >= 0]):
        hit_mats.add(int(mats_[tris["matid"][t]]["illum"]))
    assert {1, 2, 3, 7} <= hit_mats
