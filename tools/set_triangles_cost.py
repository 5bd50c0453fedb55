"""What replacing the triangles on the GPU costs, next to the host's way to a first frame, and what the pack kernel reaches next to a plain copy
(DESIGN.md §4 "Replacing the triangles"; writes profiles/set_triangles_cost.txt).

    python tools/set_triangles_cost.py [--scene sponza] [--method ploc [--radius 8]] [--steps 256] [--repeats 5] [--out profiles/set_triangles_cost.txt] [--append]

One process, the scene at 1920 x 1080 with bench.py's settings.
  1. `repeats` times, alternating: the host's way to a context (adypt_bvh_build + adypt_create, host clock each) and adypt_create_from_triangles (host
     clock, and the HIP-event parts of its staging copy, pack and build).
  2. `repeats` times: a steady-state SetTriangles — the wave pose and the rest pose in turn, the first call of each untimed — with the host clock around
     the call and the HIP-event parts: staging copy, k_pack_triangles, and the rebuild's own.
  3. k_pack_triangles' bytes per second (100 read + 128 written per triangle) next to a device-to-device copy that moves the same number of bytes
     (114 per triangle read, 114 written), HIP events around each, alternating.
  4. Windows of Trace(True, steps) after a warm-up on the tree SetTriangles left against the same tree reached by adypt_create + RebuildBVH, alternating.
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
BUILD_PARTS = ("keys", "sort", "tree", "bottom_up", "emission", "woop_nodes", "total")


def wave(p):
    q = p.astype(np.float64)
    q[..., 1] += 1.5 * np.sin(0.7 * q[..., 0]) + 0.8 * np.cos(0.9 * q[..., 2])
    q[..., 0] *= 1.1
    return q.astype(np.float32)


def table(title, names, rows):
    lines = [title, "%-52s %10s %10s %10s" % ("", "median ms", "min ms", "max ms")]
    for k, name in enumerate(names):
        v = [r[k] for r in rows]
        lines.append("%-52s %10.3f %10.3f %10.3f" % (name, statistics.median(v), min(v), max(v)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--method", choices=("linear", "ploc"), default="ploc")
    ap.add_argument("--radius", type=int, default=8, help="the search radius of --method ploc")
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_triangles_cost.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (a second scene)")
    args = ap.parse_args()
    try:
        import torch  # (its copy of the HIP runtime first, as bench.py does; also the yardstick copy of step 3)
    except ImportError:
        torch = None
    from adypt_amd import api, scenes
    os.makedirs(args.cache, exist_ok=True)
    spec = scenes.make_scene(args.scene, args.cache, width=args.width, height=args.height, pt=PT_CFG)
    cfg = api.InstanceConfig()
    assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
    scene = api.Scene()
    assert scene.LoadFromFile(cfg.m_obj_filename)
    rest = np.array(scene.triangles).view(TRI_DT)
    moved = rest.copy()
    moved["p"] = wave(rest["p"])
    n = len(rest)
    how = dict(method=args.method, radius=args.radius)
    label = "linear tree" if args.method == "linear" else "PLOC tree, radius %d" % args.radius
    cam = api.Camera()
    cam.Initialize(cfg, cfg.m_width, cfg.m_height)
    ip, iv = cam.matrices()

    def tracer(bvh):
        hs = api.HipScene()
        hs.Initialize(scene, bvh)
        p = api.HipPathTracer()
        p.Initialize(cfg.pt_params(12345), hs, cfg.m_width, cfg.m_height, cfg=cfg.bvh_params(), **how)
        p.SetCamera(ip, iv, cam.position)
        return p

    # ---- 1. the way to a context
    tracer(None).destroy()  # untimed: the code objects are loaded
    host, ours, info, sizes = [], [], None, None
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        bvh = api.WideBVH()
        bvh.Build(scene, cfg.bvh_params())
        t1 = time.perf_counter()
        p = tracer(bvh)
        t2 = time.perf_counter()
        p.destroy()
        host.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3])
        sizes = (len(bvh.nodes) // 80, len(bvh.tri_indices))
        t0 = time.perf_counter()
        p = tracer(None)
        ms = (time.perf_counter() - t0) * 1e3
        info, s, b = p.build_info, p.GetSetTrianglesTiming(), p.GetRebuildTiming()
        ours.append([ms, s["stage"], s["pack"], b["total"]])
        p.destroy()

    # ---- 2. SetTriangles in the steady state
    p = tracer(None)
    for t in (moved, rest):
        p.SetTriangles(t, cfg.bvh_params(), **how)
    steady = []
    for k in range(args.repeats):
        t0 = time.perf_counter()
        p.SetTriangles(moved if k % 2 == 0 else rest, cfg.bvh_params(), **how)
        ms = (time.perf_counter() - t0) * 1e3
        s, b = p.GetSetTrianglesTiming(), p.GetRebuildTiming()
        steady.append([ms, s["stage"], s["pack"]] + [b[key] for key in BUILD_PARTS])
    if n <= 2000000:
        lin = api.WideBVH()
        plain = api.Scene.FromArrays(moved if (args.repeats - 1) % 2 == 0 else rest, scene.materials)
        (lin.BuildPLOC(plain, cfg.bvh_params(), args.radius) if args.method == "ploc" else lin.BuildLinear(plain, cfg.bvh_params()))
        nodes, _ = p.ReadBVH()
        assert np.array_equal(nodes, lin.nodes) and np.array_equal(p.ReadTriIndices(), lin.tri_indices), "the device's tree is not the host's"
        assert p.ReadTriangles().tobytes() == np.ascontiguousarray(plain.triangles).tobytes(), "the device's triangles are not the input"
        verdict = "equal the host's tree of the same triangles byte for byte, and ReadTriangles() the input"
    else:
        verdict = "not compared (more than 2 M triangles)"

    # ---- 3. the pack kernel next to a copy of the same traffic
    traffic = n * 228
    copies = None
    if torch is not None and torch.cuda.is_available():
        src = torch.empty(n * 114, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        src.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        copies = []
        for k in range(args.repeats + 1):
            e0.record()
            dst.copy_(src)
            e1.record()
            e1.synchronize()
            if k:
                copies.append(e0.elapsed_time(e1))
            p.SetTriangles(moved if k % 2 else rest, cfg.bvh_params(), **how)  # (alternating with the kernel; its times are those of step 2)
    pack_ms = statistics.median(r[2] for r in steady)

    # ---- 4. the step rate on the tree
    p.SetTriangles(moved, cfg.bvh_params(), **how)
    host_bvh = api.WideBVH()
    host_bvh.Build(scene, cfg.bvh_params())
    q = tracer(host_bvh)
    q.UpdateTriangles(0, moved["p"].reshape(-1, 9))
    q.RebuildBVH(cfg.bvh_params(), **how)

    def window(t):
        t.Reset()
        t.Trace(True, WARMUP)
        t0 = time.perf_counter()
        t.Trace(True, args.steps)
        return (time.perf_counter() - t0) * 1e3

    tracers = (("SetTriangles", p), ("adypt_create + UpdateTriangles + RebuildBVH", q))
    rate = {name: [] for name, _ in tracers}
    for _, t in tracers:
        window(t)
    for _ in range(args.repeats):
        for name, t in tracers:
            rate[name].append(window(t))

    lines = ["Cost of replacing the triangles: %s (%d triangles), %d x %d, %d bounces, %s; %d repeats, the variants alternating in one run." % (
                 args.scene, n, args.width, args.height, PT_CFG["maxBounce"], label, args.repeats),
             "the host's SBVH tree: %d nodes, %d references; built on the GPU from the triangles: %d nodes, %d references, %d levels" % (
                 sizes[0], sizes[1], info["n_nodes"], info["n_refs"], info["levels"]),
             "After SetTriangles the device's node and index arrays " + verdict + ".", ""]
    lines += table("The way to a context (host clock):", ["adypt_bvh_build", "adypt_create", "both"], host)
    lines += [""] + table("adypt_create_from_triangles (the first row is the host clock; the others HIP events inside it):",
                          ["host clock", "staging copy (100 B per triangle)", "k_pack_triangles", "the build (device total)"], ours)
    lines += ["host build + create over create_from_triangles, medians: %.1f x" % (statistics.median(r[2] for r in host) / statistics.median(r[0] for r in ours)), ""]
    tree_rows = ["radix tree", "bottom-up (boxes, counts, DP)"] if args.method == "linear" else ["PLOC rounds", "(no pass of its own)"]
    lines += table("One SetTriangles in the steady state, the scene's own count (the first row is the host clock around the call; the others HIP events):",
                   ["host clock", "staging copy (100 B per triangle)", "k_pack_triangles", "build: centroid box + keys", "build: sort"] + ["build: " + r for r in tree_rows] +
                   ["build: emission", "build: Woop + node records", "build: device total"], steady)
    lines += ["", "k_pack_triangles: %d bytes read + %d written = %.2f MB in %.4f ms (median): %.1f GB/s" % (n * 100, n * 128, traffic / 1e6, pack_ms, traffic / pack_ms / 1e6)]
    if copies:
        c = statistics.median(copies)
        lines += ["device-to-device copy of %d bytes (the same %.2f MB moved): %.4f ms (median of %d, min %.4f, max %.4f): %.1f GB/s; kernel / copy = %.2f" % (
                      n * 114, traffic / 1e6, c, len(copies), min(copies), max(copies), traffic / c / 1e6, pack_ms / c)]
    else:
        lines += ["device-to-device copy: not measured (no torch in this environment)"]
    lines += ["", "Step rate in the wave pose: window = %d warm-up + %d timed frames, host clock around Trace(True, %d)." % (WARMUP, args.steps, args.steps),
              "%-52s %10s %10s %10s %12s" % ("", "median ms", "min ms", "max ms", "steps / s")]
    for name, v in rate.items():
        lines.append("%-52s %10.2f %10.2f %10.2f %12.1f" % (name, statistics.median(v), min(v), max(v), args.steps / (statistics.median(v) * 1e-3)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("\n" if args.append else "") + text)
    for _, t in tracers:
        t.destroy()


if __name__ == "__main__":
    main()
