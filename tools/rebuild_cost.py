"""What a new tree for a moved scene costs on the GPU, next to the host's way, and what the three trees are worth afterwards (DESIGN.md §4 "Rebuilding on
the GPU"; writes profiles/rebuild_cost.txt).

    python tools/rebuild_cost.py [--scene sponza] [--method linear|ploc [--radius 8] [--split-budget 0]] [--steps 256] [--repeats 5] [--out profiles/rebuild_cost.txt] [--append]

One process, the scene at 1920 x 1080 with bench.py's settings, in the wave pose of the tests (y += 1.5 sin(0.7 x) + 0.8 cos(0.9 z); x *= 1.1).  Three
contexts are held side by side:
    refitted   the config's tree (spatial splits), UpdateTriangles to the pose
    rebuilt    the same, then RebuildBVH: the linear tree (--method linear) or the PLOC tree (--method ploc) built on the GPU; --split-budget B
               (ploc only): with large triangles split into several references first, at most B * n more than triangles
    sbvh       adypt_bvh_build of the moved triangles + adypt_create: the parent commit's only way to a new tree
  1. `repeats` times: one RebuildBVH (HIP-event parts and the host clock around the call), and adypt_bvh_build + adypt_create (host clock).
  2. The device's arrays after the rebuild against WideBVH.BuildLinear / BuildPLOC of the moved triangles (skipped above 2 M triangles: the host build is
     slow).  (The rounds a PLOC tree takes are counted without a GPU by tools/tree_quality.py.)
  3. Windows of Trace(True, steps) after a warm-up, the three contexts alternating, `repeats` times.
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
PARTS = ("keys", "sort", "tree", "bottom_up", "emission", "woop_nodes", "total")


def wave(p):
    q = p.astype(np.float64)
    q[..., 1] += 1.5 * np.sin(0.7 * q[..., 0]) + 0.8 * np.cos(0.9 * q[..., 2])
    q[..., 0] *= 1.1
    return q.astype(np.float32)


def table(title, names, rows):
    lines = [title, "%-44s %10s %10s %10s" % ("", "median ms", "min ms", "max ms")]
    for k, name in enumerate(names):
        v = [r[k] for r in rows]
        lines.append("%-44s %10.3f %10.3f %10.3f" % (name, statistics.median(v), min(v), max(v)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--method", choices=("linear", "ploc"), default="linear")
    ap.add_argument("--radius", type=int, default=8, help="the search radius of --method ploc")
    ap.add_argument("--split-budget", type=float, default=0.0, help="of --method ploc: split large triangles first (csrc/device/presplit.hpp)")
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebuild_cost.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (a second scene)")
    args = ap.parse_args()
    if args.split_budget and args.method != "ploc":
        ap.error("--split-budget needs --method ploc")
    try:
        import torch  # noqa: F401  (its copy of the HIP runtime first, as bench.py does)
    except ImportError:
        pass
    from adypt_amd import api, scenes
    os.makedirs(args.cache, exist_ok=True)
    spec = scenes.make_scene(args.scene, args.cache, width=args.width, height=args.height, pt=PT_CFG)

    def instance():
        inst = api.Instance()
        assert inst.InitializeFromFile(spec.config_path, shift_seed=12345), api.InstanceConfig.last_error()
        return inst

    a, b = instance(), instance()
    cfg = a.m_config
    rest = np.array(a.scene.triangles).view(TRI_DT)
    moved = rest.copy()
    moved["p"] = wave(rest["p"])
    pos = moved["p"].reshape(-1, 9)
    a.m_path_tracer.UpdateTriangles(0, pos)
    b.m_path_tracer.UpdateTriangles(0, pos)
    how = dict(method=args.method, radius=args.radius)
    label = "linear tree" if args.method == "linear" else "PLOC tree, radius %d" % args.radius
    if args.split_budget:
        how["split_budget"] = args.split_budget
    info = b.m_path_tracer.RebuildBVH(cfg.bvh_params(), **how)  # untimed: the scratch is allocated, the code object is loaded
    if args.split_budget:
        label += ", split budget %g (level %d, %d triangles split)" % ((args.split_budget,) + b.m_path_tracer.GetRebuildPresplit())

    def host_way():
        t0 = time.perf_counter()
        plain = api.Scene.FromArrays(moved, a.scene.materials)
        bvh = api.WideBVH()
        bvh.Build(plain, cfg.bvh_params())
        t1 = time.perf_counter()
        sc = api.Scene()
        sc.triangles, sc.materials, sc.textures = plain.triangles, a.scene.materials, a.scene.textures
        hs = api.HipScene()
        hs.Initialize(sc, bvh)
        p = api.HipPathTracer()
        p.Initialize(cfg.pt_params(12345), hs, cfg.m_width, cfg.m_height)
        ip, iv = a.m_camera.matrices()
        p.SetCamera(ip, iv, a.m_camera.position)
        t2 = time.perf_counter()
        return p, (t1 - t0) * 1e3, (t2 - t1) * 1e3, len(bvh.nodes) // 80, len(bvh.tri_indices)

    rebuild, host, sbvh = [], [], None
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        b.m_path_tracer.RebuildBVH(cfg.bvh_params(), **how)
        ms = (time.perf_counter() - t0) * 1e3
        t = b.m_path_tracer.GetRebuildTiming()
        rebuild.append([ms] + [t[k] for k in PARTS])
        if sbvh is not None:
            sbvh[0].destroy()
        sbvh = host_way()
        host.append([sbvh[1], sbvh[2]])
    verdict = "not compared (more than 2 M triangles)"
    if len(rest) <= 2000000:
        plain = api.Scene.FromArrays(moved, a.scene.materials)
        lin = api.WideBVH()
        if args.method == "ploc":
            lin.BuildPLOC(plain, cfg.bvh_params(), args.radius, args.split_budget)
        else:
            lin.BuildLinear(plain, cfg.bvh_params())
        nodes, woop = b.m_path_tracer.ReadBVH()
        want = api.woop_matrices(moved, lin.tri_indices)
        nan = np.isnan(want)
        same = (np.array_equal(nodes, lin.nodes) and np.array_equal(b.m_path_tracer.ReadTriIndices(), lin.tri_indices) and np.array_equal(np.isnan(woop), nan)
                and np.array_equal(woop.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
        boxes = b.m_path_tracer.ReadRefBoxes() if args.split_budget else None
        same = same and (boxes is None) == (len(lin.ref_boxes) == 0) and (boxes is None or np.array_equal(boxes.view(np.uint32), lin.ref_boxes.view(np.uint32)))
        assert same, "the device's tree is not the host's (%s)" % label
        verdict = "equal WideBVH.%s + woop_matrices of the moved triangles byte for byte (host: %.0f ms tree, %.0f ms collapse and boxes)" % (
            "BuildPLOC" if args.method == "ploc" else "BuildLinear", lin.build_info.sbvh_ms, lin.build_info.wide_ms)

    def window(p):
        p.Reset()
        p.Trace(True, WARMUP)
        t0 = time.perf_counter()
        p.Trace(True, args.steps)
        return (time.perf_counter() - t0) * 1e3

    tracers = (("refitted tree (splits, refit to the pose)", a.m_path_tracer), ("rebuilt on the GPU (%s)" % label, b.m_path_tracer), ("SBVH built on the host for the pose", sbvh[0]))
    rate = {name: [] for name, _ in tracers}
    for _, p in tracers:
        window(p)
    for _ in range(args.repeats):
        for name, p in tracers:
            rate[name].append(window(p))
    lines = ["Cost of a new tree in the wave pose: %s (%d triangles), %d x %d, %d bounces; %d repeats, the variants alternating in one run." % (
                 args.scene, len(rest), args.width, args.height, PT_CFG["maxBounce"], args.repeats),
             "config's tree: %d nodes, %d references; rebuilt on the GPU (%s): %d nodes, %d references, %d levels, binary depth %d; SBVH for the pose: %d nodes, %d references" % (
                 len(a.bvh.nodes) // 80, len(a.bvh.tri_indices), label, info["n_nodes"], info["n_refs"], info["levels"], info["binary_depth"], sbvh[3], sbvh[4]),
             "After RebuildBVH the device's node, index and Woop arrays " + verdict + ".", ""]
    tree_rows = ["radix tree", "bottom-up (boxes, counts, DP)"] if args.method == "linear" else ["PLOC rounds (tree, boxes, counts, DP; one 8-byte read each)", "(no pass of its own)"]
    lines += table("One RebuildBVH, " + label + " (HIP events; the first row is the host clock around the call, allocation of the new arrays and one 4-byte read per level in it):",
                   ["host clock", "centroid box + keys", "sort (rocPRIM, 62 bits)"] + tree_rows + ["emission (every level)", "Woop + node records", "device total"], rebuild)
    lines += [""] + table("The parent commit's way to a new tree (host clock):", ["adypt_bvh_build", "adypt_create"], host)
    both = statistics.median(r[0] + r[1] for r in host)
    lines += ["build + create, median of the sums: %.1f ms = %.1f x RebuildBVH's host clock" % (both, both / statistics.median(r[0] for r in rebuild)), ""]
    lines += ["Step rate in the wave pose: window = %d warm-up + %d timed frames, host clock around Trace(True, %d)." % (WARMUP, args.steps, args.steps),
              "%-44s %10s %10s %10s %12s" % ("", "median ms", "min ms", "max ms", "steps / s")]
    for name, v in rate.items():
        lines.append("%-44s %10.2f %10.2f %10.2f %12.1f" % (name, statistics.median(v), min(v), max(v), args.steps / (statistics.median(v) * 1e-3)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(("\n" if args.append else "") + text)
    for _, p in tracers:
        p.destroy()


if __name__ == "__main__":
    main()
