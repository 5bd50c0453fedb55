"""What a moments call (Denoise(temporal=True, moments=True): variance from temporal luminance moments, from 1 spp per pose) costs next to the plain
temporal call, and that it costs nothing when unused — DESIGN.md §4 "Variance from temporal moments"; writes profiles/moments_cost.txt.

    python tools/moments_cost.py --parent-tree DIR [--repeats 7] [--steps 256] [--out profiles/moments_cost.txt]

DIR is a built checkout of the parent commit (its own adypt_amd package and libadypt_hip.so).  Two worker processes hold one context each — the
parent's library and this tree's — on the bench scene at 1920 x 1080 with bench.py's settings.  HIP events, medians of `repeats`, each series after one
untimed call of its kind, every measured call with commit=False on the same inputs.  Within one run, this tree:
  (a) the first moments call at 1 spp with no history: every hit pixel asks its window, every workgroup with a hit pixel stages its halo.  Beside it
      the plain temporal call without history at 2 spp (its merge stage: k_temporal_merge<false, false>).
  (b) the steady state: `--poses` (4) poses 1.5 degrees of yaw apart rendered at 1 spp and committed, the last 1.5 degrees from the bench camera, then
      the bench camera at 1 spp.  (One committed pose does not make a steady state at 1 spp per pose: a history is kMomentsMinLength = 4 samples long
      after four.)  Beside it the plain temporal call at 2 spp after ONE pose 1.5 degrees away was committed at 2 spp, as tools/denoise_cost.py measures it.
  For each: k_moments_variance alone (GetDenoiseMoments()["variance_ms"]), and merge + variance (GetDenoiseMergeMs()) against the plain call's merge
  stage; how many pixels took the window and how many workgroups staged (from the read-outs, on the host); the byte model beside the times.
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
GROUP_X, GROUP_Y, RADIUS = 32, 8, 3  # the workgroup of k_moments_variance (kAtrousX, kAtrousY) and kMomentsRadius
STEP_YAW = 1.5


def worker(tree, scene, width, height, cache):
    """Serves one context over stdin / stdout: one command per line, one answer per line."""
    sys.path.insert(0, tree)
    try:
        import torch  # noqa: F401  (its copy of the HIP runtime first, as bench.py does)
    except ImportError:
        pass
    import numpy as np
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
        elif cmd[0] == "setup":  # setup HISTORY_POSES SPP: plain temporal history of that many poses, then the bench camera at SPP; one untimed call of each kind
            pt.Reset()
            pt.SetNoiseStats(True)
            pt.ResetDenoiseHistory()
            for k in range(int(cmd[1]), 0, -1):
                pose(k, int(cmd[2]))
                pt.Denoise(temporal=True)
            pose(0, int(cmd[2]))
            pt.Denoise()
            pt.Denoise(temporal=True, commit=False)
            print("ok", flush=True)
        elif cmd[0] == "plain":  # -> device total of Denoise()'s events, sha1 of the result
            out = pt.Denoise()
            print("%.4f %s" % (pt.GetDenoiseTiming()["total"], sha(out)), flush=True)
        elif cmd[0] == "temporal":  # -> merge stage, device total with it, sha1 of the result
            out = pt.Denoise(temporal=True, commit=False)
            ms = pt.GetDenoiseMergeMs()
            print("%.4f %.4f %s" % (ms, pt.GetDenoiseTiming()["total"] + ms, sha(out)), flush=True)
        elif cmd[0] == "moments":  # moments HISTORY_POSES REPEATS -> variance ms ... | merge ms ... | spatial, hit, asking pixels, staged workgroups, workgroups, mean length, bytes
            pt.Reset()
            pt.SetNoiseStats(True)
            pt.ResetDenoiseHistory()
            for k in range(int(cmd[1]), 0, -1):
                pose(k, 1)
                pt.Denoise(temporal=True, moments=True)
            pose(0, 1)
            pt.Denoise(temporal=True, moments=True, commit=False)
            var, merge = [], []
            for _ in range(int(cmd[2])):
                pt.Denoise(temporal=True, moments=True, commit=False)
                info = pt.GetDenoiseMoments()
                var.append(info["variance_ms"])
                merge.append(pt.GetDenoiseMergeMs())
            n, hit = pt.ReadDenoiseHistory(), pt.ReadDenoiseGuides()["hit"]
            asks = hit & (n < 4)
            gy, gx = (height + GROUP_Y - 1) // GROUP_Y, (width + GROUP_X - 1) // GROUP_X
            padded = np.zeros((gy * GROUP_Y, gx * GROUP_X), bool)
            padded[:height, :width] = asks
            staged = int(padded.reshape(gy, GROUP_Y, gx, GROUP_X).any(axis=(1, 3)).sum())
            print(" ".join("%.4f" % v for v in var) + " | " + " ".join("%.4f" % v for v in merge) + " | %d %d %d %d %d %.3f %d"
                  % (info["pixels_spatial"], int(hit.sum()), int(asks.sum()), staged, gy * gx, float(n[hit].mean()), info["device_bytes"]), flush=True)
            pt.ResetDenoiseHistory()
    pt.destroy()


class Worker:
    def __init__(self, tree, args):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree, "--scene", args.scene, "--width", str(args.width), "--height", str(args.height),
                                   "--cache", args.cache], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert self._answer() == ["ready"], "a worker did not come up"

    def _answer(self):
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit("moments_cost: a worker ended early (exit code %s)" % self.p.wait())  # nothing more is started on the GPU
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
    """[(name, vgprs, sgprs, LDS bytes, scratch bytes)] of the moments kernels in denoise.hip's code object"""
    asm = os.path.join(CSRC, "build", "denoise.s")
    if not os.path.exists(asm):
        subprocess.check_call(["make", "-C", CSRC, "build/denoise.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = []
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", open(asm).read()):
        lds, name, scratch, sgpr, vgpr = m.groups()
        k = re.search(r"\d+(k_moments_variance|k_denoise_prepare_moments|k_temporal_merge_momentsILb[01]E)", name)
        if k:
            out.append((k.group(1).replace("ILb0E", "<false>").replace("ILb1E", "<true>"), int(vgpr), int(sgpr), int(lds), int(scratch)))
    return sorted(out)


def staging_bytes(width, height):
    """bytes every workgroup would read to stage its tile with the halo, clipped at the image border, 64 B per pixel (if every workgroup staged)"""
    read = 0
    for y0 in range(0, height, GROUP_Y):
        rows = min(y0 + GROUP_Y + RADIUS, height) - max(y0 - RADIUS, 0)
        for x0 in range(0, width, GROUP_X):
            read += rows * (min(x0 + GROUP_X + RADIUS, width) - max(x0 - RADIUS, 0)) * 64
    return read


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
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_cost.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.scene, args.width, args.height, args.cache)
    if not args.parent_tree:
        raise SystemExit("moments_cost: --parent-tree DIR (a built checkout of the parent commit) is needed")
    os.makedirs(args.cache, exist_ok=True)
    new = Worker(ROOT, args)
    old = Worker(os.path.abspath(args.parent_tree), args)
    trees = [("parent commit", old), ("this tree, unused", new)]
    px = args.width * args.height

    # ---- this tree: the moments call, and the plain temporal call's merge stage beside it ----
    def merge_stage(history_poses):
        new.ask("setup %d 2" % history_poses)
        return [float(new.ask("temporal")[0]) for _ in range(args.repeats)]

    def moments(history_poses):
        a = " ".join(new.ask("moments %d %d" % (history_poses, args.repeats))).split("|")
        return [float(v) for v in a[0].split()], [float(v) for v in a[1].split()], a[2].split()
    plain_a, (var_a, merge_a, info_a) = merge_stage(0), moments(0)
    plain_b, (var_b, merge_b, info_b) = merge_stage(1), moments(args.poses)
    lines = ["Variance from temporal moments: %s, %d x %d; HIP events, %d repeats each after one untimed call, commit=False on the same inputs, one run." % (args.scene, args.width, args.height, args.repeats), ""]
    stage_all = staging_bytes(args.width, args.height)
    for tag, what, plain, var, merge, info, plain_what in (
            ("(a)", "the first moments call at 1 spp, no history", plain_a, var_a, merge_a, info_a, "Denoise(temporal=True) at 2 spp without history: its merge stage"),
            ("(b)", "steady state: %d poses %.1f degrees of yaw apart committed at 1 spp each, then the bench camera at 1 spp" % (args.poses, STEP_YAW), plain_b, var_b, merge_b, info_b,
             "Denoise(temporal=True) at 2 spp after one pose %.1f degrees away committed at 2 spp: its merge stage" % STEP_YAW)):
        spatial, hit, asks, staged, groups, length, dev_bytes = int(info[0]), int(info[1]), int(info[2]), int(info[3]), int(info[4]), float(info[5]), int(info[6])
        m_var, m_merge, m_plain = statistics.median(var), statistics.median(merge), statistics.median(plain)
        model = 44 * px + stage_all * staged // groups
        lines += ["%s %s" % (tag, what),
                  "    %d of %d hit pixels asked their window (%d took its estimate), %d of %d workgroups staged their halo; mean history length on hit pixels %.2f"
                  % (asks, hit, spatial, staged, groups, length),
                  "%-74s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"),
                  row("    k_moments_variance alone (variance_ms)", var),
                  row("    merge + variance (GetDenoiseMergeMs())", merge),
                  row("    " + plain_what, plain),
                  "    merge + variance / the plain call's merge stage, medians: %.2f x; variance / plain merge: %.2f x" % (m_merge / m_plain, m_var / m_plain),
                  "    byte model of the variance kernel: 44 B per pixel (16 + 4 + 4 read, 16 + 4 written) + 64 B per staged tile pixel in the share of the workgroups that staged"
                  " = %.1f MB -> %.2f TB/s at the median" % (model / 1e6, model / (m_var * 1e-3) / 1e12), ""]
    lines += ["On the device for moments: %d bytes (4 per pixel + 512 = %d)." % (dev_bytes, 4 * px + 512), "",
              "The new kernels (gfx950, as compiled):", "%-36s %6s %6s %10s %8s" % ("", "VGPRs", "SGPRs", "LDS bytes", "scratch")]
    lines += ["%-36s %6d %6d %10d %8d" % k for k in kernel_resources()]

    # ---- unused: the two trees alternating ----
    ms, shas = {name: [] for name, _ in trees}, {name: set() for name, _ in trees}
    for _ in range(args.repeats):
        for name, w in trees:
            a = w.ask("window %d" % args.steps)
            ms[name].append(float(a[0]))
            shas[name].add(a[1])
    same = len(shas["parent commit"] | shas["this tree, unused"]) == 1
    lines += ["", "Unused: Trace(True, %d) after %d warm-up frames, the two trees alternating, %d windows each; images %s." % (args.steps, WARMUP, args.repeats, "bit-identical (sha1 %s)" % next(iter(shas["parent commit"]))[:12] if same else "DIFFER"),
              "%-74s %10s %10s %10s" % ("", "median ms", "min ms", "max ms")]
    lines += [row("    " + name, ms[name]) for name, _ in trees]
    lines.append("    this tree's median lies %s" % verdict(ms["parent commit"], statistics.median(ms["this tree, unused"])))
    for name, w in trees:
        w.ask("setup 1 2")
    calls = {("plain", name): [] for name, _ in trees}
    calls.update({("temporal", name): [] for name, _ in trees})
    call_sha = {"plain": set(), "temporal": set()}
    for _ in range(args.repeats):
        for what in ("plain", "temporal"):
            for name, w in trees:
                a = w.ask(what)
                calls[(what, name)].append(float(a[1] if what == "temporal" else a[0]))
                call_sha[what].add(a[-1])
    lines += ["", "Unused: Denoise() and Denoise(temporal=True, commit=False) at 2 spp after one pose %.1f degrees away was committed, the two trees alternating, %d calls each; the device total of the call's events." % (STEP_YAW, args.repeats)]
    for what in ("plain", "temporal"):
        lines.append("  %s: results %s" % (what, "bit-identical (sha1 %s)" % next(iter(call_sha[what]))[:12] if len(call_sha[what]) == 1 else "DIFFER"))
        lines += [row("    " + name, calls[(what, name)]) for name, _ in trees]
        lines.append("    this tree's median lies %s" % verdict(calls[(what, "parent commit")], statistics.median(calls[(what, "this tree, unused")])))
    new.close()
    old.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
