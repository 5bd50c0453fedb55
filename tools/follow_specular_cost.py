"""What the temporal merge by the virtual point costs (Denoise(temporal=True, follow_specular=K)) next to the calls it is made of — DESIGN.md §4 "Temporal
merge through mirrors and glass"; writes profiles/follow_specular_cost.txt.

    python tools/follow_specular_cost.py [--parent-tree DIR] [--scene sponza] [--spp 64] [--repeats 7] [--out profiles/follow_specular_cost.txt]

One process, the scene at 1920 x 1080 with bench.py's settings, --spp samples once.  Then `repeats` times, in turn, on the same image — each timed call
behind one untimed committing call of its own kind, which warms it up and leaves the history it then finds (a call finds no history of another kind):
    Denoise(temporal=True)                      GetDenoiseMergeMs() (k_temporal_merge) and the whole call (GetDenoiseTiming()["total"] + the merge)
    Denoise(specular_bounces=K)                 for K = 1, 4, 8: GetDenoiseSpecular()["chain_ms"] and the whole call
    Denoise(temporal=True, follow_specular=K)   for K = 1, 4, 8: the merge (k_temporal_merge_virtual), chain_ms (the unfolding instances) and the whole call
Beside them the registers and scratch of the new kernels as the compiler reports them (build/denoise.s, made here when it is missing).
Unused (with --parent-tree DIR, a built checkout of the parent commit with its own adypt_amd package and libadypt_hip.so): two worker processes hold one
context each, the parent's library and this tree's, and windows of Trace(True, 256), Denoise(), Denoise(temporal=True, commit=False) and
Denoise(specular_bounces=8) ALTERNATE between them in one run: bit-identical results (sha1), and this tree's median against the parent's own
min .. max spread.  A step that fails ends the run: nothing more is started on the GPU."""
import argparse
import hashlib
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.pose_cost import PT_CFG  # noqa: E402

CSRC = os.path.join(ROOT, "adypt_amd", "csrc")
BOUNCES = (1, 4, 8)
MERGE_BYTES, VIRTUAL_BYTES = 164, 180  # per pixel, the byte model of denoise_kernels.hpp: the virtual merge reads XV (16 B) beside the others


def row(name, v):
    return "%-84s %10.4f %10.4f %10.4f" % (name, statistics.median(v), min(v), max(v))


def kernel_resources():
    asm = os.path.join(CSRC, "build", "denoise.s")
    if not os.path.exists(asm):
        subprocess.check_call(["make", "-C", CSRC, "build/denoise.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    out = []
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        name, scratch, sgpr, vgpr = m.groups()
        short = re.search(r"(k_chain_startILb[01]E|k_chain_stepILb[01]E|k_denoise_prepare_class|k_denoise_prepare_virtual|k_temporal_merge_virtual|k_temporal_mergeILb0ELb0E)E", name)
        if short:
            out.append((short.group(1).replace("ILb0ELb0E", "<false, false>").replace("ILb0E", "<false>").replace("ILb1E", "<true>"), int(vgpr), int(sgpr), int(scratch)))
    return sorted(out)


WARMUP, UNUSED_SPP = 32, 64


def worker(tree, scene, width, height, cache):
    """Serves one context of the package in `tree` over stdin / stdout: one command per line, one answer per line (as tools/moments_cost.py's)."""
    sys.path.insert(0, tree)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    from adypt_amd import api, scenes
    assert os.path.realpath(os.path.dirname(api.__file__)).startswith(os.path.realpath(tree)), "the worker imported another tree's package"
    spec = scenes.make_scene(scene, cache, width=width, height=height, pt=PT_CFG)
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=12345), api.InstanceConfig.last_error()
    pt = inst.m_path_tracer

    def sha(a):
        return hashlib.sha1(a.tobytes()).hexdigest()
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "window":  # window STEPS -> wall-clock ms of the timed frames, sha1 of the image (statistics off, nothing denoised)
            pt.Reset()
            pt.SetNoiseStats(False)
            pt.Trace(True, WARMUP)
            t0 = time.perf_counter()
            pt.Trace(True, int(cmd[1]))
            print("%.4f %s" % ((time.perf_counter() - t0) * 1e3, sha(pt.ReadResult())), flush=True)
        elif cmd[0] == "setup":  # the image the three calls are timed on, a committed plain history under the same camera, one untimed call of each kind
            pt.Reset()
            pt.SetNoiseStats(True)
            pt.ResetDenoiseHistory()
            pt.Trace(True, UNUSED_SPP)
            pt.Denoise(temporal=True)
            pt.Denoise()
            pt.Denoise(specular_bounces=8)
            pt.Denoise(temporal=True, commit=False)
            print("ok", flush=True)
        elif cmd[0] == "plain":
            out = pt.Denoise()
            print("%.4f %s" % (pt.GetDenoiseTiming()["total"], sha(out)), flush=True)
        elif cmd[0] == "temporal":
            out = pt.Denoise(temporal=True, commit=False)
            print("%.4f %s" % (pt.GetDenoiseTiming()["total"] + pt.GetDenoiseMergeMs(), sha(out)), flush=True)
        elif cmd[0] == "specular":
            out = pt.Denoise(specular_bounces=8)
            print("%.4f %s" % (pt.GetDenoiseTiming()["total"], sha(out)), flush=True)
    pt.destroy()


class Worker:
    def __init__(self, tree, args):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree, "--scene", args.scene, "--width", str(args.width), "--height", str(args.height),
                                   "--cache", args.cache], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert self._answer() == ["ready"], "a worker did not come up"

    def _answer(self):
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit("follow_specular_cost: a worker ended early (exit code %s)" % self.p.wait())  # nothing more is started on the GPU
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


def unused(args):
    """the lines of the section "unused": the parent's tree and this one alternating in one run"""
    trees = [("parent commit", Worker(os.path.abspath(args.parent_tree), args)), ("this tree, unused", Worker(ROOT, args))]
    lines = []
    try:
        ms, shas = {n: [] for n, _ in trees}, {n: set() for n, _ in trees}
        for r in range(args.repeats + 1):
            for n, w in trees:
                t, h = w.ask("window %d" % args.steps)
                if r:
                    ms[n].append(float(t))
                shas[n].add(h)
        same = len(shas["parent commit"] | shas["this tree, unused"]) == 1
        lines += ["", "Unused: Trace(True, %d) after %d warm-up frames, the two trees alternating, %d windows each, wall-clock; images %s." % (args.steps, WARMUP, args.repeats, "bit-identical" if same else "DIFFER")]
        lines += [row("    " + n, ms[n]) for n, _ in trees]
        lines.append("    this tree's median lies %s" % verdict(ms["parent commit"], statistics.median(ms["this tree, unused"])))
        for _, w in trees:
            assert w.ask("setup") == ["ok"]
        for what, title in (("plain", "Denoise()"), ("temporal", "Denoise(temporal=True, commit=False), a committed history under the same camera"), ("specular", "Denoise(specular_bounces=8)")):
            ms, shas = {n: [] for n, _ in trees}, {n: set() for n, _ in trees}
            for r in range(args.repeats + 1):
                for n, w in trees:
                    t, h = w.ask(what)
                    if r:
                        ms[n].append(float(t))
                    shas[n].add(h)
            same = len(shas["parent commit"] | shas["this tree, unused"]) == 1
            lines += ["", "Unused: %s at %d spp, the whole call, HIP events, alternating, %d each; results %s." % (title, UNUSED_SPP, args.repeats, "bit-identical" if same else "DIFFER")]
            lines += [row("    " + n, ms[n]) for n, _ in trees]
            lines.append("    this tree's median lies %s" % verdict(ms["parent commit"], statistics.median(ms["this tree, unused"])))
    finally:
        for _, w in trees:
            w.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", metavar="TREE")
    ap.add_argument("--parent-tree")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "follow_specular_cost.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.scene, args.width, args.height, args.cache)
    try:
        import torch  # noqa: F401  (its copy of the HIP runtime first, as bench.py does)
    except ImportError:
        pass
    from adypt_amd import api, scenes
    os.makedirs(args.cache, exist_ok=True)
    spec = scenes.make_scene(args.scene, args.cache, width=args.width, height=args.height, pt=PT_CFG)
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=12345), api.InstanceConfig.last_error()
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    p.Trace(True, args.spp)

    def whole():
        return p.GetDenoiseTiming()["total"] + p.GetDenoiseMergeMs()

    keys = ["temporal"] + ["specular%d" % k for k in BOUNCES] + ["followed%d" % k for k in BOUNCES]
    merge, chain, total = ({k: [] for k in keys} for _ in range(3))
    info = {}
    for r in range(args.repeats + 1):
        p.Denoise(temporal=True)
        p.Denoise(temporal=True, commit=False)
        if r:
            merge["temporal"].append(p.GetDenoiseMergeMs())
            total["temporal"].append(whole())
        for k in BOUNCES:
            p.Denoise(specular_bounces=k)
            if r:
                i = p.GetDenoiseSpecular()
                assert i["bounces"] == k
                chain["specular%d" % k].append(i["chain_ms"])
                total["specular%d" % k].append(p.GetDenoiseTiming()["total"])
            p.Denoise(temporal=True, follow_specular=k)
            p.Denoise(temporal=True, follow_specular=k, commit=False)
            if r:
                i, v = p.GetDenoiseSpecular(), p.GetDenoiseVirtual()
                assert i["bounces"] == k and v["bounces"] == k
                chain["followed%d" % k].append(i["chain_ms"])
                merge["followed%d" % k].append(p.GetDenoiseMergeMs())
                total["followed%d" % k].append(whole())
                info[k] = (i, v)
    p.destroy()

    px = args.width * args.height
    med = statistics.median
    lines = ["Temporal merge through mirrors and glass: %s, %d x %d, %d spp; %d repeats, the calls in turn in one run on the same image.  HIP events unless said." % (args.scene, args.width, args.height, args.spp, args.repeats),
             "Every timed temporal call finds the history its own kind committed just before it, under the same camera.", "",
             "%-84s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"),
             row("Denoise(temporal=True): the merge stage (k_temporal_merge<false, false>)", merge["temporal"]),
             row("  the whole call (capture, prepare, merge, 5 levels)", total["temporal"])]
    for k in BOUNCES:
        i, v = info[k]
        f, s = "followed%d" % k, "specular%d" % k
        lines += ["", row("Denoise(temporal=True, follow_specular=%d): the merge stage (k_temporal_merge_virtual)" % k, merge[f]),
                  "  merge / plain temporal merge, medians: %.3f x; the byte model: %d B / %d B per pixel = %.3f x" % (med(merge[f]) / med(merge["temporal"]), VIRTUAL_BYTES, MERGE_BYTES, VIRTUAL_BYTES / MERGE_BYTES),
                  row("  chain_ms, the unfolding instances", chain[f]),
                  row("  Denoise(specular_bounces=%d): chain_ms" % k, chain[s]),
                  "  unfolding chain / chain, medians: %.3f x (the other's min .. max is %.3f .. %.3f x its median)" % (med(chain[f]) / med(chain[s]), min(chain[s]) / med(chain[s]), max(chain[s]) / med(chain[s])),
                  row("  the whole call", total[f]),
                  row("  Denoise(specular_bounces=%d): the whole call" % k, total[s]),
                  "  whole call / Denoise(temporal=True): %.3f x; / Denoise(specular_bounces=%d): %.3f x" % (med(total[f]) / med(total["temporal"]), k, med(total[f]) / med(total[s])),
                  "  followed %d pixels (class >= 2), %d of them with history; rays %d; device bytes of the virtual points, XV and counters %d (16 per local pixel + 16 per image pixel + 1024; %d pixels)"
                  % (v["pixels_followed"], v["pixels_with_history"], i["rays"], v["device_bytes"], px)]
    lines += ["", "The kernels (gfx950, as compiled):", "%-40s %6s %6s %8s" % ("", "VGPRs", "SGPRs", "scratch")]
    lines += ["%-40s %6d %6d %8d" % k for k in kernel_resources()]
    if args.parent_tree:
        lines += unused(args)
    else:
        lines += ["", "Unused: not measured in this run (no --parent-tree)."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
