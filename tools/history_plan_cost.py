"""What history-aware sampling (PlanByHistory / TraceByHistory: every block traced only as far as its history falls short) costs and saves, and that it
costs nothing when unused — DESIGN.md §4 "History-aware sampling"; writes profiles/history_plan_cost.txt.

    python tools/history_plan_cost.py --parent-tree DIR [--repeats 7] [--steps 256] [--out profiles/history_plan_cost.txt]

DIR is a built checkout of the parent commit (its own adypt_amd package and libadypt_hip.so).  Two worker processes hold one context each — the
parent's library and this tree's — on the bench scene at 1920 x 1080 with bench.py's settings.  Medians of `repeats`, each series after one untimed call of
its kind.  Within one run, this tree: `--poses` (4) poses 1.5 degrees of yaw apart rendered at `--pose-spp` (16) and committed by a plain temporal call,
the last 1.5 degrees from the bench camera; then at the bench camera, the variants ALTERNATING:
  (a) PlanByHistory(target): capture_ms and reach_ms (HIP events) against the guides stage and GetDenoiseMergeMs() of a plain temporal call
      (commit=False) at the same camera in the same run; the reach kernel's time against the byte model;
  (b) TraceByHistory(target) against Trace(True, target) from 0 spp, host clock around the call (both end with the stream drained): pixel-samples
      against target x pixels, the set changes (distinct counts - 1), the time per million pixel-samples of both;
  for every (target, step) of --targets and --steps-of-plan.
Unused: Trace(True, steps), Denoise() and Denoise(temporal=True, commit=False) at 2 spp, the two trees ALTERNATING in one run: bit-identical results
(sha1), and this tree's median against the parent's own min .. max spread.
A step that fails ends the run: nothing more is started on the GPU."""
import argparse
import hashlib
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adypt_amd", "csrc")
PT_CFG = {"maxBounce": 8, "subpixel": 8, "clamp": 4.0, "sun": [12.0, 11.0, 10.0], "stackSize": 24, "tmpLifetime": 16}  # bench.py's
WARMUP = 32
STEP_YAW = 1.5


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
    pt, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c

    def pose(k, spp):
        """the camera k steps of yaw from the bench camera, a seed of its own, spp frames from 0"""
        pt.Reset()
        pt.SetConfig(cfg.pt_params(12345 + k))
        ip, iv = api.camera_matrices(c.fov, c.yaw + STEP_YAW * k, c.pitch, width, height)
        pt.SetCamera(ip, iv, inst.m_camera.position)
        if spp:
            pt.Trace(True, spp)

    def sha(a):
        return hashlib.sha1(a.tobytes()).hexdigest()
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "window":  # window STEPS -> ms of the timed frames, sha1 of the image (statistics off, nothing denoised)
            pt.Reset()
            pt.SetNoiseStats(False)
            pose(0, WARMUP)
            t0 = time.perf_counter()
            pt.Trace(True, int(cmd[1]))
            print("%.4f %s" % ((time.perf_counter() - t0) * 1e3, sha(pt.ReadResult())), flush=True)
        elif cmd[0] == "setup":  # setup HISTORY_POSES SPP MAIN_SPP: a plain temporal history of that many poses, then the bench camera at MAIN_SPP; one untimed call of each kind
            pt.Reset()
            pt.SetNoiseStats(True)
            pt.ResetDenoiseHistory()
            for k in range(int(cmd[1]), 0, -1):
                pose(k, int(cmd[2]))
                pt.Denoise(temporal=True)
            pose(0, int(cmd[3]))
            if int(cmd[3]) >= 2:
                pt.Denoise()
                pt.Denoise(temporal=True, commit=False)
            print("ok", flush=True)
        elif cmd[0] == "plain":  # -> device total of Denoise()'s events, sha1 of the result
            out = pt.Denoise()
            print("%.4f %s" % (pt.GetDenoiseTiming()["total"], sha(out)), flush=True)
        elif cmd[0] == "temporal":  # -> merge stage, device total with it, guides stage, sha1 of the result
            out = pt.Denoise(temporal=True, commit=False)
            ms, t = pt.GetDenoiseMergeMs(), pt.GetDenoiseTiming()
            print("%.4f %.4f %.4f %s" % (ms, t["total"] + ms, t["guides"], sha(out)), flush=True)
        elif cmd[0] == "plan":  # plan TARGET STEP -> capture ms, reach ms, pixel_samples, pixels, with history, mean reach, distinct wants, device bytes (at 0 spp)
            pose(0, 0)
            info = pt.PlanByHistory(int(cmd[1]), max_spp=max(64, int(cmd[1])), step=int(cmd[2]))
            want = pt.ReadSamplePlan()[1]
            print("%.4f %.4f %d %d %d %.4f %d %d" % (info["capture_ms"], info["reach_ms"], info["pixel_samples"], info["pixels"], info["pixels_with_history"], info["mean_reach"],
                                                   len(set(int(v) for v in want)), info["device_bytes"]), flush=True)
        elif cmd[0] == "by_history":  # by_history TARGET STEP -> host ms of TraceByHistory from 0 spp, pixel_samples, distinct wants
            pose(0, 0)
            pt.DeviceSynchronize()
            t0 = time.perf_counter()
            info = pt.TraceByHistory(int(cmd[1]), max_spp=max(64, int(cmd[1])), step=int(cmd[2]))
            ms = (time.perf_counter() - t0) * 1e3
            print("%.4f %d %d" % (ms, info["pixel_samples"], len(set(int(v) for v in pt.ReadSamplePlan()[1]))), flush=True)
        elif cmd[0] == "uniform":  # uniform TARGET -> host ms of Trace(True, TARGET) from 0 spp
            pose(0, 0)
            pt.DeviceSynchronize()
            t0 = time.perf_counter()
            pt.Trace(True, int(cmd[1]))
            print("%.4f" % ((time.perf_counter() - t0) * 1e3), flush=True)
    pt.destroy()


class Worker:
    def __init__(self, tree, args):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree, "--scene", args.scene, "--width", str(args.width), "--height", str(args.height),
                                   "--cache", args.cache], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert self._answer() == ["ready"], "a worker did not come up"

    def _answer(self):
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit("history_plan_cost: a worker ended early (exit code %s)" % self.p.wait())  # nothing more is started on the GPU
        return line.split()

    def ask(self, text):
        self.p.stdin.write(text + "\n")
        self.p.stdin.flush()
        return self._answer()

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=120)


def verdict(parent, median):
    """where this tree's median lies against the parent's own windows"""
    if median < min(parent):
        return "BELOW the parent's own min .. max spread"
    return "INSIDE the parent's own min .. max spread" if median <= max(parent) else "ABOVE the parent's own min .. max spread by %.4f ms (%.2f %%)" % (median - max(parent), 100.0 * (median / max(parent) - 1.0))


def row(name, v):
    return "%-74s %10.4f %10.4f %10.4f" % (name, statistics.median(v), min(v), max(v))


def kernel_resources():
    """[(name, vgprs, sgprs, LDS bytes, scratch bytes)] of the kernels in history_plan.hip's code object"""
    asm = os.path.join(CSRC, "build", "history_plan.s")
    if not os.path.exists(asm):
        subprocess.check_call(["make", "-C", CSRC, "build/history_plan.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = []
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", open(asm).read()):
        lds, name, scratch, sgpr, vgpr = m.groups()
        k = re.search(r"\d+(k_history_reachILb[01]E)", name)
        if k:
            out.append((k.group(1).replace("ILb0E", "<false>").replace("ILb1E", "<true>"), int(vgpr), int(sgpr), int(lds), int(scratch)))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", metavar="TREE")
    ap.add_argument("--parent-tree")
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--poses", type=int, default=4)
    ap.add_argument("--pose-spp", type=int, default=16)
    ap.add_argument("--targets", default="16,32")
    ap.add_argument("--steps-of-plan", default="2,4,8")
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_plan_cost.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.scene, args.width, args.height, args.cache)
    if not args.parent_tree:
        raise SystemExit("history_plan_cost: --parent-tree DIR (a built checkout of the parent commit) is needed")
    os.makedirs(args.cache, exist_ok=True)
    new = Worker(ROOT, args)
    old = Worker(os.path.abspath(args.parent_tree), args)
    trees = [("parent commit", old), ("this tree, unused", new)]
    pixels = args.width * args.height
    lines = ["history-aware sampling: %s %d x %d, bench.py's settings; medians of %d; history: %d poses %.1f degrees apart at %d spp, committed by the plain temporal call"
             % (args.scene, args.width, args.height, args.repeats, args.poses, STEP_YAW, args.pose_spp), ""]
    try:
        # ---- this tree: the plan and the trace by it ----
        assert new.ask("setup %d %d 2" % (args.poses, args.pose_spp)) == ["ok"]
        merge, guides = [], []
        plans = {}
        combos = [(int(t), int(s)) for t in args.targets.split(",") for s in args.steps_of_plan.split(",")]
        for t, s in combos:
            new.ask("plan %d %d" % (t, s))  # untimed
        for _ in range(args.repeats):
            for t, s in combos:
                plans.setdefault((t, s), []).append(new.ask("plan %d %d" % (t, s)))
        # the plain temporal call at the same camera, same history, alternating with a plan
        for _ in range(args.repeats):
            new.ask("uniform 2")
            a = new.ask("temporal")
            merge.append(float(a[0])); guides.append(float(a[2]))
            new.ask("plan %d %d" % combos[0])
        lines += ["%-74s %10s %10s %10s" % ("this tree, ms (HIP events)", "median", "min", "max"), row("plain temporal call: guides stage (three camera launches)", guides),
                  row("plain temporal call: merge stage (k_temporal_merge<false, false>)", merge)]
        first = plans[combos[0]]
        capture, reach = [float(a[0]) for a in first], [float(a[1]) for a in first]
        lines += [row("PlanByHistory: capture_ms (the same three launches, at 0 spp)", capture), row("PlanByHistory: reach_ms (k_history_reach<false>)", reach)]
        hits = int(first[0][4])
        lines += ["", "byte model: a hit pixel reads 64 B of its own guides and at most 4 x 64 B of history (neighbours share taps: about 64 B reach memory where the motion is",
                  "smooth) and writes 4 B; the merge moves 164 B per pixel.  reach / merge = %.2f measured; (64 + 64 + 4) / 164 = %.2f by the model, (64 + 256 + 4) / 164 = %.2f at the most."
                  % (statistics.median(reach) / statistics.median(merge), 132 / 164.0, 324 / 164.0),
                  "pixels with at least one sample of history: %d of %d; mean reach %.2f; device bytes of the plan %d" % (hits, pixels, float(first[0][5]), int(first[0][7])), ""]
        lines += ["%-8s %-6s %16s %10s %8s %14s %14s %12s %12s" % ("target", "step", "pixel_samples", "share", "changes", "by history ms", "uniform ms", "ms/Mps hist", "ms/Mps unif")]
        for t, s in combos:
            new.ask("by_history %d %d" % (t, s)); new.ask("uniform %d" % t)  # untimed
            hist_ms, flat_ms, info = [], [], None
            for _ in range(args.repeats):
                info = new.ask("by_history %d %d" % (t, s))
                hist_ms.append(float(info[0]))
                flat_ms.append(float(new.ask("uniform %d" % t)[0]))
            ps, distinct = int(info[1]), int(info[2])
            h, f = statistics.median(hist_ms), statistics.median(flat_ms)
            lines.append("%-8d %-6d %16d %10.3f %8d %14.3f %14.3f %12.4f %12.4f" % (t, s, ps, ps / float(t * pixels), distinct - 1, h, f, h / (ps / 1e6), f / (t * pixels / 1e6)))
        lines += ["(host clock around the call, from 0 spp to the stream drained; TraceByHistory includes the capture, the reach kernel and the plan; a set change costs one",
                  "camera launch and one k_gather_blocks)", ""]
        lines += ["kernel resources (gfx950):"] + ["  %-28s %3d VGPRs %3d SGPRs %5d B LDS %3d B scratch" % k for k in kernel_resources()] + [""]
        # ---- unused: the two trees alternating ----
        for name, w in trees:
            w.ask("window %d" % args.steps)
        frames = {name: [] for name, _ in trees}
        shas = {name: set() for name, _ in trees}
        for _ in range(args.repeats):
            for name, w in trees:
                a = w.ask("window %d" % args.steps)
                frames[name].append(float(a[0])); shas[name].add(a[1])
        for name, w in trees:
            assert w.ask("setup 1 2 2") == ["ok"]
        plain = {name: [] for name, _ in trees}
        temporal = {name: [] for name, _ in trees}
        psha = {name: set() for name, _ in trees}
        tsha = {name: set() for name, _ in trees}
        for _ in range(args.repeats):
            for name, w in trees:
                a = w.ask("plain"); plain[name].append(float(a[0])); psha[name].add(a[1])
                a = w.ask("temporal"); temporal[name].append(float(a[1])); tsha[name].add(a[3])
        lines += ["%-74s %10s %10s %10s" % ("unused: the parent commit's library and this tree alternating, ms", "median", "min", "max")]
        for what, series, sh in (("Trace(True, %d)" % args.steps, frames, shas), ("Denoise()", plain, psha), ("Denoise(temporal=True, commit=False)", temporal, tsha)):
            for name, _ in trees:
                lines.append(row("%s: %s" % (what, name), series[name]))
            same = len(set.union(*sh.values())) == 1
            lines.append("  -> %s; results %s" % (verdict(series["parent commit"], statistics.median(series["this tree, unused"])), "BIT-IDENTICAL" if same else "DIFFER"))
    finally:
        new.close(); old.close()
    text = "\n".join(lines) + "\n"
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
