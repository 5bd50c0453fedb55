"""What moving the geometry costs, next to what it cost before (DESIGN.md §4 "Moving geometry"; writes profiles/refit_cost.txt).

    python tools/refit_cost.py [--parent-tree DIR] [--scene sponza] [--steps 256] [--repeats 7] [--out profiles/refit_cost.txt]

One worker process per tree holds a context on the scene at 1920 x 1080, 8 bounces (bench.py's settings).  The pose is the wave of the tests
(y += 1.5 sin(0.7 x) + 0.8 cos(0.9 z); x *= 1.1), normals kept.
  1. This tree: `repeats` times, alternating, (a) one whole-scene UpdateTriangles — the HIP-event parts (adypt_get_refit_timing) and the host clock around
     the call — and (b) what the parent commit needs for the same change: adypt_bvh_build of the moved triangles plus adypt_create, host clock.
  2. The step rate after the pose: windows of Trace(True, steps) alternating between the refitted context and a context created on a tree REBUILT from the
     moved triangles.  Whether the two images agree bit for bit is written down, not required: where two triangles are hit at the same t (abutting and
     overlapping faces) the closest hit is the one the traversal meets first, and the two trees order their nodes differently.
  3. Unused (needs --parent-tree, a built checkout of the parent commit): windows of Trace(True, steps) alternating between the parent and this tree,
     UpdateTriangles never called; this tree's median is to lie inside the parent's own min .. max spread.
Every answer of a worker is waited for under a time limit; the first failure ends the run and nothing more is started on the GPU."""
import argparse
import hashlib
import os
import select
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_CFG = {"maxBounce": 8, "subpixel": 8, "clamp": 4.0, "sun": [12.0, 11.0, 10.0], "stackSize": 24, "tmpLifetime": 16}  # bench.py's
WARMUP = 32
STEP_LIMIT_S = 600  # per answer


def wave(p):
    """p: [n, 3, 3] float32 positions"""
    q = p.astype(np.float64)
    q[..., 1] += 1.5 * np.sin(0.7 * q[..., 0]) + 0.8 * np.cos(0.9 * q[..., 2])
    q[..., 0] *= 1.1
    return q.astype(np.float32)


def worker(tree, scene, width, height, cache):
    """Serves one context over stdin / stdout: one command per line, one answer per line."""
    sys.path.insert(0, tree)
    try:
        import torch  # noqa: F401  (its copy of the HIP runtime first, as bench.py does)
    except ImportError:
        pass
    from adypt_amd import api, scenes
    assert os.path.realpath(os.path.dirname(api.__file__)).startswith(os.path.realpath(tree)), "the worker imported another tree's package"
    spec = scenes.make_scene(scene, cache, width=width, height=height, pt=PT_CFG)
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=12345), api.InstanceConfig.last_error()
    pt = inst.m_path_tracer
    cfg = inst.m_config
    tri_dt = np.dtype([("p", "<f4", (3, 3)), ("n", "<f4", (3, 3)), ("tc", "<f4", (3, 2)), ("matid", "<i4")])
    rest = np.array(inst.scene.triangles).view(tri_dt)
    moved = rest.copy()
    moved["p"] = wave(rest["p"])
    other = {}  # the context on the rebuilt tree

    def window(p, steps):
        p.Reset()
        p.Trace(True, WARMUP)
        t0 = time.perf_counter()
        p.Trace(True, steps)
        ms = (time.perf_counter() - t0) * 1e3
        return ms, hashlib.sha1(p.ReadResult().tobytes()).hexdigest()

    def rebuilt_context():
        """adypt_bvh_build + adypt_create for the moved triangles: (tracer, build ms, create ms)"""
        t0 = time.perf_counter()
        plain = api.Scene.FromArrays(moved, inst.scene.materials)
        bvh = api.WideBVH()
        bvh.Build(plain, cfg.bvh_params())
        t1 = time.perf_counter()
        sc = api.Scene()
        sc.triangles, sc.materials, sc.textures = plain.triangles, inst.scene.materials, inst.scene.textures
        hs = api.HipScene()
        hs.Initialize(sc, bvh)
        p = api.HipPathTracer()
        p.Initialize(cfg.pt_params(12345), hs, cfg.m_width, cfg.m_height)
        ip, iv = inst.m_camera.matrices()
        p.SetCamera(ip, iv, inst.m_camera.position)
        t2 = time.perf_counter()
        return p, (t1 - t0) * 1e3, (t2 - t1) * 1e3

    print("ready tris %d refs %d nodes %d" % (len(rest), len(inst.bvh.tri_indices), len(inst.bvh.nodes) // 80), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "window":  # window STEPS -> ms, sha1 (this context as it is)
            print("%.4f %s" % window(pt, int(cmd[1])), flush=True)
        elif cmd[0] == "refit":  # one whole-scene update to the wave pose -> host ms, scatter, references + Woop, nodes, total
            pt.UpdateTriangles(0, rest["p"].reshape(-1, 9))  # (back to the rest pose first, untimed: every timed update moves every vertex)
            t0 = time.perf_counter()
            pt.UpdateTriangles(0, moved["p"].reshape(-1, 9))
            host = (time.perf_counter() - t0) * 1e3
            t = pt.GetRefitTiming()
            print("%.4f %.4f %.4f %.4f %.4f" % (host, t["scatter"], t["references_woop"], t["nodes"], t["total"]), flush=True)
        elif cmd[0] == "verify":  # the device's arrays in the moved pose against the host's refit of the same tree -> "same" or what differs
            b = api.WideBVH()
            b.nodes, b.tri_indices = np.array(inst.bvh.nodes), inst.bvh.tri_indices
            sc = api.Scene()
            sc.triangles = moved.view(np.uint8).reshape(-1)
            b.Refit(sc)
            want = api.woop_matrices(moved, b.tri_indices)
            nodes, woop = pt.ReadBVH()
            nan = np.isnan(want)  # (degenerate triangles: NaN on both sides, the NaN's sign is the processor's)
            ok_w = np.array_equal(np.isnan(woop), nan) and np.array_equal(woop.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
            print("same" if np.array_equal(nodes, b.nodes) and ok_w else "differ:%s%s" % ("" if np.array_equal(nodes, b.nodes) else "nodes", "" if ok_w else "woop"), flush=True)
        elif cmd[0] == "rebuild":  # the parent's way to the same pose -> build ms, create ms; the context is kept for "window_rebuilt"
            if "pt" in other:
                other.pop("pt").destroy()
            p, build_ms, create_ms = rebuilt_context()
            other["pt"] = p
            print("%.4f %.4f" % (build_ms, create_ms), flush=True)
        elif cmd[0] == "window_rebuilt":
            print("%.4f %s" % window(other["pt"], int(cmd[1])), flush=True)
    for p in list(other.values()) + [pt]:
        p.destroy()


class Worker:
    def __init__(self, tree, args):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree, "--scene", args.scene, "--width", str(args.width), "--height", str(args.height),
                                   "--cache", args.cache], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        self.ready = self._answer()
        assert self.ready and self.ready[0] == "ready", "a worker did not come up"

    def _answer(self):
        if not select.select([self.p.stdout], [], [], STEP_LIMIT_S)[0]:
            self.p.kill()
            raise SystemExit("refit_cost: a worker did not answer within %d s" % STEP_LIMIT_S)  # nothing more is started on the GPU
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit("refit_cost: a worker ended early (exit code %s)" % self.p.wait())
        return line.split()

    def ask(self, text):
        self.p.stdin.write(text + "\n")
        self.p.stdin.flush()
        return self._answer()

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
            self.p.wait(timeout=120)
        except (OSError, subprocess.TimeoutExpired):
            self.p.kill()


def table(title, names, rows):
    lines = [title, "%-44s %10s %10s %10s" % ("", "median ms", "min ms", "max ms")]
    for k, name in enumerate(names):
        v = [r[k] for r in rows]
        lines.append("%-44s %10.3f %10.3f %10.3f" % (name, statistics.median(v), min(v), max(v)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", metavar="TREE")
    ap.add_argument("--parent-tree")
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit_cost.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.scene, args.width, args.height, args.cache)
    os.makedirs(args.cache, exist_ok=True)
    new = Worker(ROOT, args)
    old = Worker(os.path.abspath(args.parent_tree), args) if args.parent_tree else None
    refit, rebuild, rate = [], [], {"refitted tree": [], "rebuilt tree": []}
    unused = {"parent commit": [], "this tree, unused": []}
    sha = {}
    try:
        if old:  # before anything moves: both trees hold the rest pose
            pairs = [("parent commit", old), ("this tree, unused", new)]
            for name, w in pairs:
                w.ask("window 64")
            for _ in range(args.repeats):
                for name, w in pairs:
                    t, h = w.ask("window %d" % args.steps)
                    unused[name].append(float(t))
                    assert sha.setdefault("rest", h) == h, "%s: the rest pose rendered differently" % name
        new.ask("refit")  # untimed: the plan is made, the arrays are allocated, the code object is loaded
        verdict = new.ask("verify")[0]
        assert verdict == "same", "the device's refit is not the host's: " + verdict
        for _ in range(args.repeats):
            refit.append([float(v) for v in new.ask("refit")])
            rebuild.append([float(v) for v in new.ask("rebuild")])
        for cmd in ("window 64", "window_rebuilt 64"):
            new.ask(cmd)
        for _ in range(args.repeats):
            for name, cmd in (("refitted tree", "window"), ("rebuilt tree", "window_rebuilt")):
                t, h = new.ask("%s %d" % (cmd, args.steps))
                rate[name].append(float(t))
                assert sha.setdefault(name, h) == h, "%s: two windows gave different images" % name
    finally:
        new.close()
        if old:
            old.close()
    lines = ["Cost of moving every vertex: %s (%s triangles, %s references, %s nodes), %d x %d, %d bounces; %d repeats, the variants alternating in one run."
             % (args.scene, new.ready[2], new.ready[4], new.ready[6], args.width, args.height, PT_CFG["maxBounce"], args.repeats), ""]
    lines += ["After the update the device's node and Woop arrays equal the host's adypt_bvh_refit + adypt_woop_matrices of the moved triangles.", ""]
    lines += table("One whole-scene UpdateTriangles (HIP events; the first row is the host clock around the call, the upload of 36 B per triangle in it):",
                   ["host clock", "upload + scatter", "per-reference records + Woop", "nodes (every level)", "device total"], refit)
    lines += [""] + table("The same change before this feature (host clock):", ["adypt_bvh_build", "adypt_create"], rebuild)
    both = statistics.median(r[0] + r[1] for r in rebuild)
    lines += ["rebuild + create, median of the sums: %.1f ms = %.0f x the update's host clock" % (both, both / statistics.median(r[0] for r in refit)), ""]
    lines += ["Step rate in the moved pose: window = %d warm-up + %d timed frames, host clock around Trace(True, %d); the two images are %s." % (
                  WARMUP, args.steps, args.steps, "bit-identical" if sha["refitted tree"] == sha["rebuilt tree"] else "not bit-identical (hits at equal t go to the triangle met first; the trees differ in order)"),
              "%-20s %10s %10s %10s %12s" % ("", "median ms", "min ms", "max ms", "steps / s")]
    for name, v in rate.items():
        lines.append("%-20s %10.2f %10.2f %10.2f %12.1f" % (name, statistics.median(v), min(v), max(v), args.steps / (statistics.median(v) * 1e-3)))
    lines.append("the refitted tree runs at %.3f of the rebuilt tree's step rate" % (statistics.median(rate["rebuilt tree"]) / statistics.median(rate["refitted tree"])))
    lines.append("")
    if old:
        lines += ["Unused (UpdateTriangles never called): the same windows, the two trees alternating in one run; images bit-identical (sha1 %s)." % sha["rest"][:12],
                  "%-20s %10s %10s %10s" % ("", "median ms", "min ms", "max ms")]
        for name, v in unused.items():
            lines.append("%-20s %10.2f %10.2f %10.2f" % (name, statistics.median(v), min(v), max(v)))
        p, n = unused["parent commit"], statistics.median(unused["this tree, unused"])
        lines.append("this tree's median lies %s the parent's own min .. max spread" % ("INSIDE" if min(p) <= n <= max(p) else "OUTSIDE"))
    else:
        lines.append("Unused against the parent commit: not measured (no --parent-tree).")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
