"""The smallest hand-made scenes of the specular-guide tests (not a test module): a few quads placed in the camera's own frame, so that what a
scene is named after does not depend on which way the camera happens to look.  Each comes as arrays: TRI_DT triangles, MAT_DT materials, textures."""
import numpy as np

from adypt_amd import api
from oracle import oracle_py as O

FOV, YAW, PITCH = 60.0, 30.0, -10.0
MIRROR, GLASS, WALL, TEXTURED = 0, 1, 2, 3


def materials():
    m = np.zeros(4, O.MAT_DT)
    m["dtex"] = m["etex"] = m["stex"] = -1
    m["dissolve"], m["ior"] = 1.0, 1.0
    m["illum"][MIRROR], m["ks"][MIRROR] = 3, (0.9, 0.8, 0.7)
    m["illum"][GLASS], m["ior"][GLASS], m["ks"][GLASS] = 7, 1.5, (1.0, 1.0, 1.0)
    m["illum"][WALL], m["kd"][WALL] = 1, (0.6, 0.5, 0.4)
    m["illum"][TEXTURED], m["kd"][TEXTURED], m["dtex"][TEXTURED] = 1, (0.2, 0.2, 0.2), 0
    return m


def texture():
    return np.random.RandomState(3).randint(0, 256, size=(8, 8, 3)).astype(np.uint8)


def camera_frame(w, h):
    """(forward, right, up) of the pixel-centre camera ray through the middle of the image, from the matrices the tracer is given"""
    ip, iv = api.camera_matrices(FOV, YAW, PITCH, w, h)
    m, v = ip.astype(np.float64), iv.astype(np.float64)

    def direction(sx, sy):
        t = m[0:3] * sx + m[4:7] * sy + m[8:11] + m[12:15]
        r = v[0:3] * t[0] + v[4:7] * t[1] + v[8:11] * t[2]
        return r / np.linalg.norm(r)
    f = direction(0.0, 0.0)
    r = direction(0.5, 0.0) - f
    r -= f * np.dot(r, f)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    return f, r, u


def through(tris, w, h, x, y):
    """the direction in which pixel (x, y) sees `tris` from the origin: asked of the oracle's position frame, not worked out here"""
    host = api.Scene.FromArrays(tris, materials())
    b = api.WideBVH()
    b.Build(host, api.InstanceConfig().bvh_params())
    ip, iv = api.camera_matrices(FOV, YAW, PITCH, w, h)
    P = O.make_params(w, h, [0.0, 0.0, 0.0], ip, iv)
    p = O.primary_frame(O.Scene(b.nodes, b.tri_indices, tris, materials()), P, 5)[0][y, x, :3].astype(np.float64)
    return p / np.linalg.norm(p)


def quad(centre, ex, ey, normal, mat):
    """two triangles spanning centre +- ex +- ey with one normal and texture coordinates (0, 0) .. (3, 3) (the texture repeats)"""
    c, ex, ey = (np.asarray(a, np.float64) for a in (centre, ex, ey))
    p = [c - ex - ey, c + ex - ey, c + ex + ey, c - ex + ey]
    tc = [(0, 0), (3, 0), (3, 3), (0, 3)]
    t = np.zeros(2, O.TRI_DT)
    for k, idx in enumerate(((0, 1, 2), (0, 2, 3))):
        t["p"][k] = [p[i] for i in idx]
        t["n"][k] = [normal] * 3
        t["tc"][k] = [tc[i] for i in idx]
        t["matid"][k] = mat
    return t


def scene(name, w, h):
    """-> (triangles, materials, textures, camera position)"""
    f, r, u = camera_frame(w, h)
    pos = np.zeros(3, np.float32)
    big = 50.0
    front_mirror = quad(3.0 * f, big * r, big * u, -f, MIRROR)
    if name == "facing_mirrors":  # a mirror fills the view, another stands behind the camera: no chain ever ends by itself
        tris = [front_mirror, quad(-3.0 * f, big * r, big * u, f, MIRROR)]
    elif name == "mirror_under_sky":  # ... and nothing behind the camera
        tris = [front_mirror]
    elif name == "glass_box":  # the camera inside a long glass box: the side walls are met at grazing angles (total internal reflection), the far wall head-on
        s, near, far = 0.5, -1.0, 20.0
        mid, half = 0.5 * (near + far), 0.5 * (far - near)
        tris = [quad(far * f, s * r, s * u, f, GLASS), quad(near * f, s * r, s * u, -f, GLASS),
                quad(mid * f + s * r, half * f, s * u, r, GLASS), quad(mid * f - s * r, half * f, s * u, -r, GLASS),
                quad(mid * f + s * u, half * f, s * r, u, GLASS), quad(mid * f - s * u, half * f, s * r, -u, GLASS)]
    elif name == "mirror_shows_texture":  # behind the camera a textured wall, seen in the mirror
        tris = [front_mirror, quad(-3.0 * f, big * r, big * u, f, TEXTURED)]
    elif name == "one_chain_pixel":  # a diffuse wall with a mirror the size of a pixel in front of its middle
        s = 0.3 * (2.0 * 2.5 * np.tan(np.radians(FOV) / 2) / max(w, h))  # under a third of a pixel at that distance, whichever axis the field of view spans
        wall = quad(3.0 * f, big * r, big * u, -f, WALL)
        tris = [wall, quad(2.5 * through(wall, w, h, w // 2, h // 2), s * r, s * u, -f, MIRROR)]
    else:
        raise KeyError(name)
    return np.concatenate(tris), materials(), [texture()], pos


class Built:
    """a hand-made scene as the library and as the oracle take it"""

    def __init__(self, name, w, h):
        self.name, self.w, self.h = name, w, h
        self.tris, self.mats, self.textures, self.pos = scene(name, w, h)
        host = api.Scene.FromArrays(self.tris, self.mats)
        self.bvh = api.WideBVH()
        self.bvh.Build(host, api.InstanceConfig().bvh_params())
        self.scene = api.Scene()
        self.scene.triangles, self.scene.materials, self.scene.textures = host.triangles, host.materials, self.textures
        self.ip, self.iv = api.camera_matrices(FOV, YAW, PITCH, w, h)

    def pt_params(self, seed=5):
        p = api.InstanceConfig().pt_params(seed)
        p.stack_size, p.max_bounce, p.subpixel, p.tmp_lifetime = 32, 4, 1, 4
        return p

    def oracle(self, tris=None):
        p = self.pt_params()
        osc = O.Scene(self.bvh.nodes, self.bvh.tri_indices, self.tris if tris is None else tris, self.mats, textures=self.textures)
        P = O.make_params(self.w, self.h, [float(x) for x in self.pos], self.ip, self.iv, stack_size=p.stack_size, max_bounce=p.max_bounce, subpixel=p.subpixel,
                          tmp_life=p.tmp_lifetime, tmin=p.ray_tmin, clamp=p.clamp, sun=list(p.sun))
        return osc, P

    def tracer(self, cls=None, **kw):
        hs = api.HipScene()
        hs.Initialize(self.scene, self.bvh)
        t = (cls or api.HipPathTracer)()
        t.Initialize(self.pt_params(), hs, self.w, self.h, **kw)
        t.SetCamera(self.ip, self.iv, self.pos)
        return t
