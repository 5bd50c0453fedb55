"""What the tests of the temporal merge by the virtual point share (not a test module): the planar hand scene — a mirror that fills the view and a
diffuse wall behind the camera, so that every pixel's chain is one bounce long and its virtual point can be derived: the mirror image of the wall; a
lamp overhead, which no camera sees in the mirror, lights the wall (between two facing planes next to no path reaches the sky) — its cameras a step apart, and what the CPU oracle gives for one pose of any scene.  The scene is made of tests/specular_scenes.py's pieces."""
import numpy as np

from adypt_amd import api
from oracle import oracle_py as O
from tests import noise_truth as T
from tests import specular_scenes as SC
from tests import specular_truth as S

STEP_YAW, STEP_MOVE = 1.5, 0.15  # a step of the camera, as in tests/test_temporal_definition.py
MIRROR_AT, WALL_AT = 3.0, -3.0   # along the first camera's forward axis
LAMP_AT, LAMP = 8.0, 4           # along its up axis: far above what the mirror shows of the wall at these fields of view; the lamp's material index


class Planar(SC.Built):
    """SC.Built of the planar scene; camera(k) is k steps on: STEP_MOVE to the side (the first camera's right axis) and STEP_YAW of yaw each."""

    def __init__(self, w, h):  # (SC.Built's own __init__ makes the scenes SC.scene names; this is none of them)
        self.name, self.w, self.h = "mirror_shows_wall", w, h
        f, r, u = SC.camera_frame(w, h)
        self.frame = (f, r, u)
        big = 50.0
        self.tris = np.concatenate([SC.quad(MIRROR_AT * f, big * r, big * u, -f, SC.MIRROR), SC.quad(WALL_AT * f, big * r, big * u, f, SC.WALL),
                                    SC.quad(LAMP_AT * u, 12.0 * r, 3.0 * f, -u, LAMP)])
        lamp = np.zeros(1, O.MAT_DT)
        lamp["dtex"] = lamp["etex"] = lamp["stex"] = -1
        lamp["dissolve"], lamp["ior"], lamp["illum"], lamp["ke"] = 1.0, 1.0, 1, (6.0, 5.0, 4.0)
        self.mats, self.textures, self.pos = np.concatenate([SC.materials(), lamp]), [SC.texture()], np.zeros(3, np.float32)
        host = api.Scene.FromArrays(self.tris, self.mats)
        self.bvh = api.WideBVH()
        self.bvh.Build(host, api.InstanceConfig().bvh_params())
        self.scene = api.Scene()
        self.scene.triangles, self.scene.materials, self.scene.textures = host.triangles, host.materials, self.textures
        self.ip, self.iv = api.camera_matrices(SC.FOV, SC.YAW, SC.PITCH, w, h)

    def camera(self, k):
        """(position, inv_proj, inv_view) of camera k"""
        pos = (STEP_MOVE * k * self.frame[1]).astype(np.float32)
        ip, iv = api.camera_matrices(SC.FOV, SC.YAW + STEP_YAW * k, SC.PITCH, self.w, self.h)
        return pos, ip, iv

    def oracle_at(self, k):
        """(oracle scene, oracle parameters) under camera k"""
        p = self.pt_params()
        pos, ip, iv = self.camera(k)
        osc = O.Scene(self.bvh.nodes, self.bvh.tri_indices, self.tris, self.mats, textures=self.textures)
        P = O.make_params(self.w, self.h, [float(x) for x in pos], ip, iv, stack_size=p.stack_size, max_bounce=p.max_bounce, subpixel=p.subpixel,
                          tmp_life=p.tmp_lifetime, tmin=p.ray_tmin, clamp=p.clamp, sun=list(p.sun))
        return osc, P

    def mirror_image(self, point):
        """fp64: `point` (..., 3) reflected in the mirror's plane"""
        f = self.frame[0]
        p = np.asarray(point, np.float64)
        return p - 2.0 * ((p @ f) - MIRROR_AT)[..., None] * f


def oracle_pose(osc, P, seed, sobol_matrices, spp, frames=None, ref_spp=0):
    """What the oracle gives for one pose: image, m2 and spp (the filter's inputs after spp frames), primary (S.primary_guides), images (after every one
    of `frames` frames), cam (origin, inv_proj, inv_view as the tracer is given them) and, with ref_spp, ref: the image after ref_spp frames."""
    w, h = P.width, P.height
    shift = O.shift_bytes(seed, w, h)
    _, m2 = T.moments(T.frame_samples(osc, P, shift, sobol_matrices, spp))
    state, images = O.PathTracerState(w, h), []
    for _ in range(frames or spp):
        O.pt_frames(osc, P, shift, sobol_matrices, state, 1)
        images.append(state.accum[..., :3].copy())
    out = dict(image=images[spp - 1], m2=m2, spp=spp, images=images, primary=S.primary_guides(osc, P))
    if ref_spp:
        O.pt_frames(osc, P, shift, sobol_matrices, state, ref_spp - state.spp)
        out["ref"] = state.accum[..., :3].copy()
    return out


_tiny0 = {}


def tiny0(scene_cache, w=100, h=75, life=16, sub=3):
    """(oracle scene, the scene's config record) of tiny0 at that size, once; camera_params moves the record's camera"""
    key = (w, h, life, sub)
    if key not in _tiny0:
        from adypt_amd import scenes
        spec = scenes.make_scene("tiny0", scene_cache, width=w, height=h, pt={"tmpLifetime": life, "maxBounce": 6, "subpixel": sub})
        cfg = api.InstanceConfig()
        assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
        sc = api.Scene()
        assert sc.LoadFromFile(cfg.m_obj_filename)
        b = api.WideBVH()
        if not b.LoadFromFile(cfg.m_bvh_filename, cfg.bvh_params()):
            b.Build(sc, cfg.bvh_params())
            assert b.SaveToFile(cfg.m_bvh_filename, cfg.bvh_params())
        _tiny0[key] = (O.Scene(b.nodes, b.tri_indices, sc.triangles, sc.materials, textures=sc.textures), cfg, (cfg.c.yaw, list(cfg.c.position)))
    return _tiny0[key]


def tiny0_camera(entry, k, axis=0):
    """(oracle parameters, (origin, inv_proj, inv_view)) of tiny0's camera k steps on, as tests/test_temporal_definition.py moves it"""
    _, cfg, (yaw0, pos0) = entry
    c = cfg.c
    pos = list(pos0)
    pos[axis] += STEP_MOVE * k
    c.yaw = yaw0 + STEP_YAW * k
    for i in range(3):
        c.position[i] = pos[i]
    P = T.oracle_params(c)
    ip, iv = O.camera(c.fov, c.yaw, c.pitch, c.width, c.height)
    c.yaw = yaw0
    for i in range(3):
        c.position[i] = pos0[i]
    return P, (np.array(pos, np.float32), ip, iv)
