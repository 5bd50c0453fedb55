"""What a pose given by vertices costs (BindMesh + PoseVertices: 12 B per vertex cross the bus, 24 with normals) next to the route there was before
(UpdateTriangles: 72 B per triangle of positions and normals from the host) — DESIGN.md §4 "Poses given by vertices"; writes profiles/mesh_cost.txt.

    python tools/mesh_cost.py [--scene sponza] [--repeats 5] [--out profiles/mesh_cost.txt] [--append]

One process, the scene at 1920 x 1080 with bench.py's settings, welded by weld_triangles, its first tree built on the GPU (PLOC, radius 8).  Two poses
in turn: every vertex displaced by a wave of 1 % of the scene's height.  Three routes, `repeats` times, alternating, each after one untimed call of
its kind, with the host clock around the call, the HIP-event stages of GetRefitTiming() and, for the first two, of GetMeshTiming():
  (a) PoseVertices(positions): the normals computed on the device
  (b) PoseVertices(positions, normals): the normals given — those mesh_normals() computes on the host beforehand, not timed
  (c) UpdateTriangles with the arrays of the same pose, made on the host by mesh_triangles() beforehand and not timed
Afterwards the records, nodes and Woop data of the three routes are compared.  A step that fails ends the run: nothing more is started on the GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_cost import PT_CFG, STAGES, TRI_DT, table  # noqa: E402

MESH_STAGES = ("upload", "faces", "normals", "records")


def wave_poses(rest_p):
    """two sets of vertex positions: y and x displaced by a wave along x and z, up to 1 % of the scene's height"""
    p = rest_p.astype(np.float64)
    height = float(np.ptp(p[:, 1]))
    out = []
    for sign in (1.0, -1.0):
        q = p.copy()
        q[:, 1] += sign * 0.01 * height * np.sin(40.0 * p[:, 0] / height) * np.cos(30.0 * p[:, 2] / height)
        q[:, 0] += sign * 0.005 * height * np.sin(25.0 * p[:, 1] / height)
        out.append(np.ascontiguousarray(q.astype(np.float32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_cost.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (a second scene)")
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (its copy of the HIP runtime first, as bench.py does)
    except ImportError:
        pass
    from adypt_amd import api, scenes
    os.makedirs(args.cache, exist_ok=True)
    spec = scenes.make_scene(args.scene, args.cache, width=args.width, height=args.height, pt=PT_CFG)
    cfg = api.InstanceConfig()
    assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
    scene = api.Scene()
    assert scene.LoadFromFile(cfg.m_obj_filename)
    rest = np.array(scene.triangles).view(TRI_DT)
    n = len(rest)
    t0 = time.perf_counter()
    idx, rest_p, _ = api.weld_triangles(rest)
    weld_s = time.perf_counter() - t0
    nv = len(rest_p)
    positions = wave_poses(rest_p)
    normals = [api.mesh_normals(idx, p) for p in positions]                                        # (not timed)
    posed = [api.mesh_triangles(rest, idx, p, nr).view(TRI_DT) for p, nr in zip(positions, normals)]  # (the parent's route has these made on the host: not timed)
    arrays = [(np.ascontiguousarray(t["p"].reshape(-1, 9)), np.ascontiguousarray(t["n"].reshape(-1, 9))) for t in posed]
    del posed
    cam = api.Camera()
    cam.Initialize(cfg, cfg.m_width, cfg.m_height)
    ip, iv = cam.matrices()

    def tracer():
        hs = api.HipScene()
        hs.Initialize(scene, None)
        p = api.HipPathTracer()
        p.Initialize(cfg.pt_params(12345), hs, cfg.m_width, cfg.m_height, cfg=cfg.bvh_params(), method="ploc", radius=8)
        p.SetCamera(ip, iv, cam.position)
        return p

    computed, given, by_update = tracer(), tracer(), tracer()
    t0 = time.perf_counter()
    computed.BindMesh(idx, nv)
    bind_ms = (time.perf_counter() - t0) * 1e3
    given.BindMesh(idx, nv)
    binding = computed.GetMeshBinding()

    def timed(call, t, mesh):
        t0 = time.perf_counter()
        call()
        ms = (time.perf_counter() - t0) * 1e3
        s = t.GetRefitTiming()
        m = t.GetMeshTiming() if mesh else dict.fromkeys(MESH_STAGES, 0.0)
        return [ms] + [s[k] for k in STAGES] + [m[k] for k in MESH_STAGES]

    routes = (("(a) PoseVertices, normals computed", lambda k: computed.PoseVertices(positions[k % 2]), computed, True),
              ("(b) PoseVertices, normals given", lambda k: given.PoseVertices(positions[k % 2], normals[k % 2]), given, True),
              ("(c) UpdateTriangles, arrays made on the host", lambda k: by_update.UpdateTriangles(0, arrays[k % 2][0], arrays[k % 2][1]), by_update, False))
    rows = {name: [] for name, _, _, _ in routes}
    for name, call, t, mesh in routes:
        call(1)  # untimed: staging buffers, the refit plan
    for k in range(args.repeats):
        for name, call, t, mesh in routes:
            rows[name].append(timed(lambda: call(k), t, mesh))
    # (the last timed calls of the three routes were of the same pose)
    want = (by_update.ReadTriangleRecords().tobytes(),) + tuple(a.view(np.uint8).tobytes() for a in by_update.ReadBVH())
    for t in (computed, given):
        assert (t.ReadTriangleRecords().tobytes(),) + tuple(a.view(np.uint8).tobytes() for a in t.ReadBVH()) == want, "the routes left other bytes on the device"

    valence = 3.0 * n / nv
    model = {"a": 12 * nv, "b": 24 * nv, "c": 72 * n}
    lines = ["Cost of a pose given by vertices: %s (%d triangles, welded to %d vertices in %.2f s on the host: %.2f corners per vertex, max_valence %d), %d x %d, %d bounces, "
             "PLOC tree built on the GPU; every vertex moved; %d repeats, the routes alternating in one run." % (
                 args.scene, n, nv, weld_s, valence, binding["max_valence"], args.width, args.height, PT_CFG["maxBounce"], args.repeats),
             "From the host per pose, the byte model: (a) %d bytes (12 per vertex), (b) %d bytes (24 per vertex), (c) %d bytes (72 per triangle): (c) / (a) = %.2f, (c) / (b) = %.2f." % (
                 model["a"], model["b"], model["c"], model["c"] / model["a"], model["c"] / model["b"]),
             "The mesh binding holds %d bytes on the device (%.1f per triangle); BindMesh took %.1f ms on the host clock (the counting pass, the planes, the upload)." % (
                 binding["device_bytes"], binding["device_bytes"] / n, bind_ms),
             "After the last pose of the three routes the records, the nodes and the Woop data on the device are equal byte for byte.", ""]
    for name, _, _, mesh in routes:
        v = rows[name]
        first = "upload + mesh kernels" if mesh else "upload + scatter"
        stages = [("host clock", [r[0] for r in v]), (first, [r[1] for r in v])]
        if mesh:
            stages += [("    upload", [r[5] for r in v]), ("    k_mesh_faces", [r[6] for r in v]), ("    k_mesh_normals", [r[7] for r in v]), ("    k_mesh_records", [r[8] for r in v])]
        stages += [("per-reference records + Woop data", [r[2] for r in v]), ("nodes (every level)", [r[3] for r in v]), ("device total", [r[4] for r in v])]
        lines += table("%s (the first row is the host clock around the call; the others HIP events, GetRefitTiming() and GetMeshTiming()):" % name, stages) + [""]
    med = {name[1]: (statistics.median(r[0] for r in rows[name]), statistics.median(r[1] for r in rows[name])) for name, _, _, _ in routes}
    lines += ["Measured, medians, first stage (HIP events): (a) %.3f ms   (b) %.3f ms   (c) %.3f ms: (c) / (a) = %.2f, (c) / (b) = %.2f" % (
                  med["a"][1], med["b"][1], med["c"][1], med["c"][1] / med["a"][1], med["c"][1] / med["b"][1]),
              "Measured, medians, host clock: (a) %.3f ms   (b) %.3f ms   (c) %.3f ms: (c) / (a) = %.2f, (c) / (b) = %.2f" % (
                  med["a"][0], med["b"][0], med["c"][0], med["c"][0] / med["a"][0], med["c"][0] / med["b"][0])]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("\n" if args.append else "") + text)
    for t in (computed, given, by_update):
        t.destroy()


if __name__ == "__main__":
    main()
