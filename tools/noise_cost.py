"""What the noise statistics cost (DESIGN.md §4 "Noise statistics"; writes profiles/noise_stats_cost.txt).

    python tools/noise_cost.py --parent-tree DIR [--steps 512] [--repeats 7] [--out profiles/noise_stats_cost.txt]

DIR is a built checkout of the parent commit (its own adypt_amd package and libadypt_hip.so).  Two worker processes hold one context each — the
parent's library and this tree's — on the bench scene at 1920 x 1080, 8 bounces, and the timed windows ALTERNATE between three variants in one run:
parent, this tree with the statistics off, this tree with them on.  A window = Reset, 32 frames of warm-up, then `steps` frames under a host clock
(Trace returns after the stream has drained).  Every variant's median and spread (min .. max over the repeats) are reported, so that a difference
can be held against the run-to-run spread.  Then, on this tree: the time of one GetNoise() query, and TraceUntil(check_every = 16) against
Trace(True, n) to the same spp.  The images of the three variants are compared bit for bit on the way (the statistics never change the picture)."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_CFG = {"maxBounce": 8, "subpixel": 8, "clamp": 4.0, "sun": [12.0, 11.0, 10.0], "stackSize": 24, "tmpLifetime": 16}  # bench.py's
WARMUP = 32


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
    print("ready fif %d" % pt.GetFramesInFlight(), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "window":  # window on|off STEPS -> ms of the timed frames, sha1 of the image
            pt.Reset()
            if hasattr(pt, "SetNoiseStats"):
                pt.SetNoiseStats(cmd[1] == "on")
            pt.Trace(True, WARMUP)
            t0 = time.perf_counter()
            pt.Trace(True, int(cmd[2]))
            ms = (time.perf_counter() - t0) * 1e3
            print("%.4f %s" % (ms, hashlib.sha1(pt.ReadResult().tobytes()).hexdigest()), flush=True)
        elif cmd[0] == "query":  # query N -> median ms of one GetNoise() on an idle context
            ts = []
            for _ in range(int(cmd[1])):
                t0 = time.perf_counter()
                pt.GetNoise()
                ts.append((time.perf_counter() - t0) * 1e3)
            print("%.4f %.4f %.4f" % (statistics.median(ts), min(ts), max(ts)), flush=True)
        elif cmd[0] == "until":  # until N -> ms of TraceUntil(check_every 16) that runs to N spp (target 0), and of Trace(True, N), statistics on in both
            n = int(cmd[1])
            out = []
            for how in ("until", "plain"):
                pt.Reset()
                pt.SetNoiseStats(True)
                pt.Trace(True, WARMUP)
                pt.Reset()
                t0 = time.perf_counter()
                if how == "until":
                    g = pt.TraceUntil(0.0, 2, n, 16)
                    assert g["spp"] == n
                else:
                    pt.Trace(True, n)
                out.append((time.perf_counter() - t0) * 1e3)
            print("%.4f %.4f" % tuple(out), flush=True)
    pt.destroy()


class Worker:
    def __init__(self, tree, args):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree, "--scene", args.scene, "--width", str(args.width), "--height", str(args.height),
                                   "--cache", args.cache], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        self.ready = self._answer()
        assert self.ready and self.ready[0] == "ready", "a worker did not come up"

    def _answer(self):
        line = self.p.stdout.readline()
        if not line:
            raise SystemExit("noise_cost: a worker ended early (exit code %s)" % self.p.wait())  # nothing more is started on the GPU
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", metavar="TREE")
    ap.add_argument("--parent-tree")
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_stats_cost.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.scene, args.width, args.height, args.cache)
    if not args.parent_tree:
        raise SystemExit("noise_cost: --parent-tree DIR (a built checkout of the parent commit) is needed")
    os.makedirs(args.cache, exist_ok=True)
    new = Worker(ROOT, args)
    old = Worker(os.path.abspath(args.parent_tree), args)
    variants = [("parent commit", old, "off"), ("statistics off", new, "off"), ("statistics on", new, "on")]
    ms = {name: [] for name, _, _ in variants}
    sha = {}
    try:
        for name, w, mode in variants:  # one untimed window each: code objects loaded, the buffers of "on" allocated once
            w.ask("window %s %d" % (mode, 64))
        for _ in range(args.repeats):
            for name, w, mode in variants:
                t, h = w.ask("window %s %d" % (mode, args.steps))
                ms[name].append(float(t))
                assert sha.setdefault(name, h) == h, "%s: two windows gave different images" % name
        assert len(set(sha.values())) == 1, "the variants do not render the same image: %s" % sha
        new.ask("window on 64")
        q = [float(v) for v in new.ask("query 50")]
        until = [[float(v) for v in new.ask("until 256")] for _ in range(5)]
    finally:
        new.close()
        old.close()
    lines = ["Cost of the noise statistics: %s, %d x %d, %d bounces, tmpLifetime %d, %s frames in flight; window = %d warm-up + %d timed frames; %d repeats, the three variants alternating in one run."
             % (args.scene, args.width, args.height, PT_CFG["maxBounce"], PT_CFG["tmpLifetime"], new.ready[2], WARMUP, args.steps, args.repeats),
             "Host clock around Trace(True, %d) (returns after the stream has drained).  The variants' images are bit-identical (sha1 %s)." % (args.steps, next(iter(sha.values()))[:12]),
             "",
             "%-16s %10s %10s %10s %9s %11s" % ("variant", "median ms", "min ms", "max ms", "spread", "ms / frame")]
    base = statistics.median(ms["parent commit"])
    for name, _, _ in variants:
        v = ms[name]
        med = statistics.median(v)
        lines.append("%-16s %10.2f %10.2f %10.2f %8.2f%% %11.4f   (%+.2f%% against the parent's median)" % (name, med, min(v), max(v), 100.0 * (max(v) - min(v)) / med, med / args.steps, 100.0 * (med - base) / base))
    lines += ["",
              "one GetNoise() on an idle context (k_noise_blocks + a 16 B per block copy + the host formulas): median %.3f ms (min %.3f, max %.3f, 50 calls)" % tuple(q),
              "TraceUntil(target 0, check_every 16) to 256 spp against Trace(True, 256), statistics on in both, from 0 spp: median %.2f ms against %.2f ms (5 runs each, alternating): %.2f ms per check"
              % (statistics.median(u[0] for u in until), statistics.median(u[1] for u in until),
                 (statistics.median(u[0] for u in until) - statistics.median(u[1] for u in until)) / 16.0),
              "(a check ends a wavefront pass early: TraceUntil's passes are check_every frames long, a plain Trace's are frames-in-flight long)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
