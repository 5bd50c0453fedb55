"""What a pose with morph targets costs when the device makes it (BindMorph + Pose(morph_weights=...): the weights and the matrices cross the bus) next
to a pose without a layer and to the route there was before (the morph made on the host, 72 B per triangle through UpdateTriangles) — DESIGN.md §4
"Morph targets"; writes profiles/morph_cost.txt.

    python tools/morph_cost.py [--scene sponza] [--parts 16] [--targets 8] [--repeats 5] [--out profiles/morph_cost.txt]

One process, the scene at 1920 x 1080 with bench.py's settings, its first tree built on the GPU (PLOC, radius 8), the parts and matrices of
tools/pose_cost.py.  Target k displaces a run of one sixteenth of the triangles of its own along their normals.  Four routes, `repeats` times,
alternating, each after one untimed call of its kind, with the host clock around the call and the HIP-event stages of GetRefitTiming():
  (a) Pose(matrices), no layer bound
  (b) Pose(matrices, morph_weights=zeros), the layer bound
  (c) Pose(matrices, morph_weights=w), every weight non-zero
  (d) UpdateTriangles with the arrays of the same pose, made on the host by pose_triangles(..., morph=...) beforehand and not timed
Afterwards the records, nodes and Woop data of (c) and (d) are compared, and the records of one more (b) and (a).  A step that fails ends the run: nothing more is
started on the GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_cost import PT_CFG, STAGES, TRI_DT, slab_poses, table  # noqa: E402


def layer_of(rest, n_targets):
    """(triangles, targets, deltas [e, 18]): target k moves the triangles [2 k n / 16, (2 k + 1) n / 16) along their vertex normals by up to 1 % of the
    scene's height, more in the middle of the run; the normals stay"""
    n = len(rest)
    height = float(np.ptp(rest["p"][..., 1]))
    tri, tgt, d = [], [], []
    for k in range(n_targets):
        run = np.arange(2 * k * n // 16, (2 * k + 1) * n // 16)
        bump = np.sin(np.linspace(0.0, np.pi, len(run)))[:, None, None]
        delta = np.zeros((len(run), 2, 3, 3), np.float32)
        delta[:, 0] = (0.01 * height * bump * rest["n"][run]).astype(np.float32)
        tri.append(run.astype(np.int32))
        tgt.append(np.full(len(run), k, np.int32))
        d.append(delta.reshape(-1, 18))
    return np.concatenate(tri), np.concatenate(tgt), np.concatenate(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parts", type=int, default=16)
    ap.add_argument("--targets", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_cost.txt"))
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
    layer = layer_of(rest, args.targets)
    weights = [np.linspace(0.25, 1.0, args.targets).astype(np.float32), -np.linspace(0.25, 1.0, args.targets).astype(np.float32)[::-1].copy()]
    zeros = np.zeros(args.targets, np.float32)
    posed = [api.pose_triangles(rest, m, parts=parts, morph=layer, morph_weights=w).view(TRI_DT) for m, w in zip(sets, weights)]  # (not timed)
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

    plain, morphed, by_update = tracer(), tracer(), tracer()
    plain.BindParts(parts, args.parts)
    morphed.BindParts(parts, args.parts)
    morphed.BindMorph(*layer, args.targets)
    binding, info = morphed.GetPoseBinding(), morphed.GetMorphBinding()

    def timed(call, t):
        t0 = time.perf_counter()
        call()
        ms = (time.perf_counter() - t0) * 1e3
        s = t.GetRefitTiming()
        return [ms] + [s[k] for k in STAGES]

    routes = (("(a) Pose, no layer", lambda k: plain.Pose(sets[k % 2]), plain),
              ("(b) Pose, layer bound, all weights 0", lambda k: morphed.Pose(sets[k % 2], morph_weights=zeros), morphed),
              ("(c) Pose, %d weights non-zero" % args.targets, lambda k: morphed.Pose(sets[k % 2], morph_weights=weights[k % 2]), morphed),
              ("(d) UpdateTriangles, morphed on the host", lambda k: by_update.UpdateTriangles(0, arrays[k % 2][0], arrays[k % 2][1]), by_update))
    rows = {name: [] for name, _, _ in routes}
    for name, call, t in routes:
        call(1)  # untimed: staging buffers, the refit plan
    for k in range(args.repeats):
        for name, call, t in routes:
            rows[name].append(timed(lambda: call(k), t))
    # (the last timed calls of (c) and (d) were of the same pose)
    same = (morphed.ReadTriangleRecords().tobytes() == by_update.ReadTriangleRecords().tobytes() and
            all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(morphed.ReadBVH(), by_update.ReadBVH())))
    assert same, "routes (c) and (d) left other bytes on the device"
    plain.Pose(sets[0])
    morphed.Pose(sets[0], morph_weights=zeros)
    assert morphed.ReadTriangleRecords().tobytes() == plain.ReadTriangleRecords().tobytes(), "all weights 0 left other records than a pose without a layer"

    entries, active = len(layer[0]), len(layer[0])
    now, off, per_entry = 76 + 72, 8, 78
    model = {"a": n * now, "b": n * (now + off) + 4 * entries, "c": n * (now + off) + per_entry * active}
    lines = ["Cost of a pose with morph targets: %s (%d triangles), %d x %d, %d bounces, PLOC tree built on the GPU; whole-scene pose, %d parts; %d targets, %d entries on %d "
             "triangles; %d repeats, the routes alternating in one run." % (args.scene, n, args.width, args.height, PT_CFG["maxBounce"], args.parts, args.targets, entries,
                                                                           info["n_tris_touched"], args.repeats),
             "From the host per pose: (a) %d bytes (48 per matrix), (b) and (c) %d bytes more (4 per target), (d) %d bytes (72 per triangle)." % (args.parts * 48, args.targets * 4, n * 72),
             "The matrix binding holds %d bytes on the device (%.1f per triangle), the morph layer %d bytes (%.1f per entry)." % (
                 binding["device_bytes"], binding["device_bytes"] / n, info["device_bytes"], info["device_bytes"] / entries),
             "After the last (c) and (d) records, nodes and Woop data on the device are equal byte for byte; after one more (a) and (b) of one pose, their records.", ""]
    for name, _, _ in routes:
        v = rows[name]
        first = "upload + scatter" if name.startswith("(d)") else "weights, matrices + k_pose"
        lines += table("%s (the first row is the host clock around the call; the others HIP events, GetRefitTiming()):" % name,
                       [("host clock", [r[0] for r in v]), (first, [r[1] for r in v]), ("per-reference records + Woop data", [r[2] for r in v]),
                        ("nodes (every level)", [r[3] for r in v]), ("device total", [r[4] for r in v])]) + [""]
    med = {name[1]: (statistics.median(r[0] for r in rows[name]), statistics.median(r[1] for r in rows[name])) for name, _, _ in routes}
    lines += ["Byte model of k_pose, device memory traffic: per triangle 76 + 72 B as without a layer (rest pose and part read, record written), + 8 B of offsets with a layer, + 78 B per "
              "active entry (72 of deltas, 4 of target index, the weight); an entry of weight 0 costs its 4 B of index.",
              "  (a) %.1f MB   (b) %.1f MB, %.3f x (a)   (c) %.1f MB, %.3f x (a)" % (model["a"] / 1e6, model["b"] / 1e6, model["b"] / model["a"], model["c"] / 1e6, model["c"] / model["a"]),
              "Measured, medians, first stage (HIP events): (a) %.3f ms   (b) %.3f ms, %.3f x (a)   (c) %.3f ms, %.3f x (a)   (d) %.3f ms" % (
                  med["a"][1], med["b"][1], med["b"][1] / med["a"][1], med["c"][1], med["c"][1] / med["a"][1], med["d"][1]),
              "Measured, medians, host clock: (a) %.3f ms   (b) %.3f ms   (c) %.3f ms   (d) %.3f ms: (c) is %.3f ms less than (d) (%.2f x)" % (
                  med["a"][0], med["b"][0], med["c"][0], med["d"][0], med["d"][0] - med["c"][0], med["d"][0] / med["c"][0])]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    for t in (plain, morphed, by_update):
        t.destroy()


if __name__ == "__main__":
    main()
