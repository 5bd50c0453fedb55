"""What a pose costs when the device makes it (BindParts + Pose: only the matrices cross the bus) next to the route there was before
(UpdateTriangles: 72 B per triangle of positions and normals from the host) — DESIGN.md §4 "Posing on the GPU"; writes profiles/pose_cost.txt.

    python tools/pose_cost.py [--scene sponza] [--parts 16] [--steps 256] [--repeats 5] [--out profiles/pose_cost.txt] [--append]

One process, the scene at 1920 x 1080 with bench.py's settings, its first tree built on the GPU (PLOC, radius 8).  The scene is cut into `parts` slabs
along x; a pose turns every slab about its own vertical axis and lifts it, two poses in turn.
  1. `repeats` times, alternating, each after one untimed call of its kind:
       UpdateTriangles(0, positions, normals) with the posed arrays computed on the host beforehand (pose_triangles, not timed)
       Pose(matrices)
     with the host clock around the call and the HIP-event stages of GetRefitTiming().  Afterwards the records, nodes and Woop data of the two routes
     are compared.
  2. Windows of Trace(True, steps) after a warm-up, alternating between a context posed by Pose and one posed by UpdateTriangles.
A step that fails ends the run: nothing more is started on the GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PT_CFG = {"maxBounce": 8, "subpixel": 8, "clamp": 4.0, "sun": [12.0, 11.0, 10.0], "stackSize": 24, "tmpLifetime": 16}  # bench.py's
WARMUP = 32
TRI_DT = np.dtype([("p", "<f4", (3, 3)), ("n", "<f4", (3, 3)), ("tc", "<f4", (3, 2)), ("matid", "<i4")])
STAGES = ("scatter", "references_woop", "nodes", "total")


def slab_poses(rest, n_parts):
    """(part of every triangle, two sets of matrices [n_parts, 3, 4]): slabs of equal triangle count along x, turned about the vertical axis through
    their own middle by up to +-6 degrees and lifted by up to 2 % of the scene's height"""
    centre = rest["p"].astype(np.float64).mean(axis=1)
    order = np.argsort(centre[:, 0], kind="stable")
    parts = np.empty(len(rest), dtype=np.int32)
    parts[order] = (np.arange(len(rest), dtype=np.int64) * n_parts // len(rest)).astype(np.int32)
    height = float(np.ptp(rest["p"][..., 1]))
    sets = []
    for sign in (1.0, -1.0):
        mats = np.zeros((n_parts, 3, 4), dtype=np.float64)
        for k in range(n_parts):
            c = centre[parts == k].mean(axis=0)
            a = np.radians(sign * 6.0 * np.sin(1.0 + 2.0 * k))
            R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
            mats[k, :, :3] = R
            mats[k, :, 3] = c - R @ c + np.array([0.0, sign * 0.02 * height * np.cos(k), 0.0])
        sets.append(mats.astype(np.float32))
    return parts, sets


def table(title, rows_by_name):
    lines = [title, "%-44s %10s %10s %10s" % ("", "median ms", "min ms", "max ms")]
    for name, v in rows_by_name:
        lines.append("%-44s %10.3f %10.3f %10.3f" % (name, statistics.median(v), min(v), max(v)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parts", type=int, default=16)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_cost.txt"))
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
    parts, sets = slab_poses(rest, args.parts)
    posed = [api.pose_triangles(rest, m, parts=parts).view(TRI_DT) for m in sets]  # (the parent's route has these made on the host: not timed)
    arrays = [(np.ascontiguousarray(t["p"].reshape(-1, 9)), np.ascontiguousarray(t["n"].reshape(-1, 9))) for t in posed]
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

    by_pose, by_update = tracer(), tracer()
    by_pose.BindParts(parts, args.parts)
    binding = by_pose.GetPoseBinding()

    def timed(call, t):
        t0 = time.perf_counter()
        call()
        ms = (time.perf_counter() - t0) * 1e3
        s = t.GetRefitTiming()
        return [ms] + [s[k] for k in STAGES]

    routes = (("UpdateTriangles", lambda k: by_update.UpdateTriangles(0, arrays[k % 2][0], arrays[k % 2][1]), by_update),
              ("Pose", lambda k: by_pose.Pose(sets[k % 2]), by_pose))
    rows = {name: [] for name, _, _ in routes}
    for name, call, t in routes:
        call(1)  # untimed: staging buffers, the refit plan
    for k in range(args.repeats):
        for name, call, t in routes:
            rows[name].append(timed(lambda: call(k), t))
    last = (args.repeats - 1) % 2
    same = (by_pose.ReadTriangleRecords().tobytes() == by_update.ReadTriangleRecords().tobytes() and
            all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(by_pose.ReadBVH(), by_update.ReadBVH())))
    assert same, "the two routes left other bytes on the device"

    def window(t):
        t.Reset()
        t.Trace(True, WARMUP)
        t0 = time.perf_counter()
        t.Trace(True, args.steps)
        return (time.perf_counter() - t0) * 1e3

    rate = {name: [] for name, _, _ in routes}
    for _, _, t in routes:
        window(t)
    for _ in range(args.repeats):
        for name, _, t in routes:
            rate[name].append(window(t))

    lines = ["Cost of a pose: %s (%d triangles), %d x %d, %d bounces, PLOC tree built on the GPU; whole-scene pose, %d parts; %d repeats, the routes alternating in one run." % (
                 args.scene, n, args.width, args.height, PT_CFG["maxBounce"], args.parts, args.repeats),
             "From the host per pose: UpdateTriangles %d bytes (72 per triangle), Pose %d bytes (48 per matrix).  The binding holds %d bytes on the device (%.1f per triangle)." % (
                 n * 72, args.parts * 48, binding["device_bytes"], binding["device_bytes"] / n),
             "After pose %d of both routes the records, the nodes and the Woop data on the device are equal byte for byte." % last, ""]
    for name, _, _ in routes:
        v = rows[name]
        lines += table("%s (the first row is the host clock around the call; the others HIP events, GetRefitTiming()):" % name,
                       [("host clock", [r[0] for r in v]), ("upload + scatter" if name == "UpdateTriangles" else "matrices + k_pose", [r[1] for r in v]),
                        ("per-reference records + Woop data", [r[2] for r in v]), ("nodes (every level)", [r[3] for r in v]), ("device total", [r[4] for r in v])]) + [""]
    u, p = (statistics.median(r[0] for r in rows[name]) for name in ("UpdateTriangles", "Pose"))
    lines += ["host clock, medians: UpdateTriangles %.3f ms, Pose %.3f ms: %.3f ms less (%.2f x)" % (u, p, u - p, u / p), "",
              "Step rate in the last pose: window = %d warm-up + %d timed frames, host clock around Trace(True, %d)." % (WARMUP, args.steps, args.steps),
              "%-44s %10s %10s %10s %12s" % ("", "median ms", "min ms", "max ms", "steps / s")]
    for name, v in rate.items():
        lines.append("%-44s %10.2f %10.2f %10.2f %12.1f" % ("posed by " + name, statistics.median(v), min(v), max(v), args.steps / (statistics.median(v) * 1e-3)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("\n" if args.append else "") + text)
    for _, _, t in routes:
        t.destroy()


if __name__ == "__main__":
    main()
