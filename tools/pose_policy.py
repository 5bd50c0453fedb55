"""Refit or rebuild: what the tree's SAH cost says about a pose, and from which cost ratio on a rebuild pays (DESIGN.md §4 "Refit or rebuild"; writes
profiles/pose_policy.txt, which README's guidance for UpdateTriangles(rebuild_above=...) quotes).

    python tools/pose_policy.py [--scene sponza] [--steps 64] [--repeats 5] [--out profiles/pose_policy.txt]

One process, the scene at 1920 x 1080 with bench.py's settings.  Two contexts, both with a PLOC tree built on the GPU in the rest pose:
    refitted   UpdateTriangles(pose, rebuild_above=huge): the refit and the cost measurement of the policy call, never its rebuild
    rebuilt    UpdateTriangles(pose), then RebuildBVH(method="ploc"): the tree the policy would build for the pose
16 poses of growing distance from the rest pose: the wave of the tests (y += 1.5 sin(0.7 x) + 0.8 cos(0.9 z); x *= 1.1) scaled by k = 1/16 .. 1, and
every odd triangle moved along x by f times the scene's x extent, f = 0.01 .. 1.5.  Per pose, medians of `repeats`:
  1. the cost ratio refitted / as built, the policy call's cost_ms next to GetRefitTiming() of the same call;
  2. RebuildBVH on the other context: the host clock around the call, and the rebuilt tree's cost;
  3. windows of Trace(True, steps) after a warm-up on both contexts, alternating;
  4. once: nodes visited and triangles tested per ray of 2 instrumented frames on both trees (work = nodes + 0.3 triangles).
From that: the gain of a rebuild per frame, and per frame count N the cost ratio above which the rebuild is repaid within N frames.
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
WARMUP = 16
NEVER = 1e30
TRI_DT = np.dtype([("p", "<f4", (3, 3)), ("n", "<f4", (3, 3)), ("tc", "<f4", (3, 2)), ("matid", "<i4")])
WAVE_K = (1 / 16, 1 / 8, 3 / 16, 1 / 4, 3 / 8, 1 / 2, 3 / 4, 1.0)
APART_F = (0.01, 0.02, 0.05, 0.1, 0.25, 0.5, 1.0, 1.5)
FRAMES = (1, 8, 64)


def wave(p, k):
    q = p.astype(np.float64)
    w = q.copy()
    w[..., 1] += 1.5 * np.sin(0.7 * q[..., 0]) + 0.8 * np.cos(0.9 * q[..., 2])
    w[..., 0] *= 1.1
    return (q + k * (w - q)).astype(np.float32)


def apart(p, f):
    q = p.astype(np.float64)
    q[1::2, :, 0] += f * (float(p[..., 0].max()) - float(p[..., 0].min()))
    return q.astype(np.float32)


def break_even(rows, n):
    """rows sorted by ratio: (ratio, gain per frame in ms, rebuild ms).  The ratio at which n * gain first reaches the rebuild's cost, linear between
    the neighbouring poses; None when it never does."""
    prev = None
    for ratio, gain, rebuild in rows:
        net = n * gain - rebuild
        if net >= 0.0:
            if prev is None or prev[1] >= 0.0:
                return ratio
            return prev[0] + (ratio - prev[0]) * (0.0 - prev[1]) / (net - prev[1])
        prev = (ratio, net)
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_policy.txt"))
    args = ap.parse_args()
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

    ia, ib = instance(), instance()
    a, b = ia.m_path_tracer, ib.m_path_tracer
    cfg = ia.m_config.bvh_params()
    rest = np.array(ia.scene.triangles).view(TRI_DT)["p"]
    info = None
    for p in (a, b):
        info = p.RebuildBVH(cfg, "ploc")
    built = a.GetTreeCost(cfg)  # (the reference of every policy call below: measured on the tree as built)

    def window(p):
        p.Reset()
        p.Trace(True, WARMUP)
        t0 = time.perf_counter()
        p.Trace(True, args.steps)
        return (time.perf_counter() - t0) * 1e3

    def work(p):
        p.SetInstrumentation(timing=False, counters=True)
        p.Reset()
        p.ResetStats()
        p.Trace(True, 2)
        st = p.GetStats()
        p.SetInstrumentation()
        p.Reset()
        return st["nodes_visited"] / st["rays"], st["tris_tested"] / st["rays"]

    poses = [("wave k = %.4g" % k, wave(rest, k)) for k in WAVE_K] + [("apart f = %.4g" % f, apart(rest, f)) for f in APART_F]
    med = statistics.median
    rows = []
    for name, pos in poses:
        flat = pos.reshape(-1, 9)
        ratio, cost_ms, nodes_ms, refit_ms, rebuild_ms, win_a, win_b = [], [], [], [], [], [], []
        for _ in range(args.repeats):
            out = a.UpdateTriangles(0, flat, rebuild_above=NEVER, cfg=cfg)
            assert out["rebuilt"] == 0 and out["built"] == built
            t = a.GetRefitTiming()
            ratio.append(out["refitted"]["cost"] / out["built"]["cost"])
            cost_ms.append(out["cost_ms"])
            nodes_ms.append(t["nodes"])
            refit_ms.append(t["total"])
            b.UpdateTriangles(0, flat)
            t0 = time.perf_counter()
            b.RebuildBVH(cfg, "ploc")
            rebuild_ms.append((time.perf_counter() - t0) * 1e3)
            win_a.append(window(a))
            win_b.append(window(b))
        refitted_cost, rebuilt_cost = a.GetTreeCost(cfg)["cost"], b.GetTreeCost(cfg)["cost"]
        wa, wb = work(a), work(b)
        rows.append(dict(name=name, ratio=med(ratio), cost_ms=med(cost_ms), nodes_ms=med(nodes_ms), refit_ms=med(refit_ms), rebuild_ms=med(rebuild_ms), frame_a=med(win_a) / args.steps,
                         frame_b=med(win_b) / args.steps, cost_a=refitted_cost, cost_b=rebuilt_cost, work_a=wa[0] + 0.3 * wa[1], work_b=wb[0] + 0.3 * wb[1], nodes_a=wa[0], tris_a=wa[1]))
        print(rows[-1], flush=True)

    lines = ["Refit or rebuild by the tree's SAH cost: %s (%d triangles), %d x %d, %d bounces; medians of %d; window = %d warm-up + %d timed frames, host clock." % (
                 args.scene, len(rest), args.width, args.height, PT_CFG["maxBounce"], args.repeats, WARMUP, args.steps),
             "Both contexts start from the PLOC tree built on the GPU in the rest pose: %d nodes, %d references, %d levels; cost as built %.3f (inner_q %d, leaf_q %d)." % (
                 info["n_nodes"], info["n_refs"], info["levels"], built["cost"], built["inner_q"], built["leaf_q"]),
             "refitted: UpdateTriangles(pose, rebuild_above=never); rebuilt: UpdateTriangles(pose) + RebuildBVH(method=\"ploc\"), its host clock in `rebuild ms`.", "",
             "%-16s %7s %8s %8s %8s %9s %10s %10s %9s %9s %9s %9s %9s" % ("pose", "ratio", "cost ms", "nodes ms", "refit ms", "rebuild ms", "ms / frame", "ms / frame", "cost", "work/ray", "cost/work", "cost", "work/ray"),
             "%-16s %7s %8s %8s %8s %9s %10s %10s %9s %9s %9s %9s %9s" % ("", "", "", "", "", "", "refitted", "rebuilt", "refitted", "refitted", "refitted", "rebuilt", "rebuilt")]
    for r in rows:
        lines.append("%-16s %7.3f %8.4f %8.4f %8.3f %9.2f %10.3f %10.3f %9.2f %9.2f %9.2f %9.2f %9.2f" % (
            r["name"], r["ratio"], r["cost_ms"], r["nodes_ms"], r["refit_ms"], r["rebuild_ms"], r["frame_a"], r["frame_b"], r["cost_a"], r["work_a"], r["cost_a"] / r["work_a"], r["cost_b"], r["work_b"]))
    below = sum(1 for r in rows if r["cost_ms"] < r["nodes_ms"])
    lines += ["", "cost_ms against the refit's `nodes` stage of the same call (one launch reading the node array once, against one launch per level reading and writing it): "
              "cost_ms is below `nodes` in %d of %d poses; medians over the poses %.4f ms against %.4f ms." % (below, len(rows), med(r["cost_ms"] for r in rows), med(r["nodes_ms"] for r in rows)), ""]
    lines.append("Break-even: a rebuild is repaid within N frames where N x (ms / frame refitted - ms / frame rebuilt) >= rebuild ms; poses ordered by ratio, linear between neighbours.")
    ordered = sorted(rows, key=lambda r: r["ratio"])
    for n in FRAMES:
        x = break_even([(r["ratio"], r["frame_a"] - r["frame_b"], r["rebuild_ms"]) for r in ordered], n)
        lines.append("  N = %2d: %s" % (n, "above ratio %.3f a rebuild is repaid within %d frame%s" % (x, n, "" if n == 1 else "s") if x is not None else
                                        "no measured pose repays a rebuild within %d frame%s (largest ratio measured: %.3f)" % (n, "" if n == 1 else "s", ordered[-1]["ratio"])))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    for p in (a, b):
        p.destroy()


if __name__ == "__main__":
    main()
