"""What adaptive sampling saves and what it costs (DESIGN.md §4 "Adaptive sampling"; writes profiles/adaptive_sampling.txt).

    python tools/adaptive_cost.py --parent-tree DIR [--repeats 7] [--out profiles/adaptive_sampling.txt]

DIR is a built checkout of the parent commit (its own adypt_amd package and libadypt_hip.so).  Two worker processes hold one context each — the
parent's library and this tree's — on the bench scene at 1920 x 1080, 8 bounces.  First a probe on this tree: a uniform run with the block noise
read every 16 spp up to 512, from which the target is taken — the geometric mean of the worst block's noise at the two checks around --stop-at
(default 256) spp, so that the uniform TraceUntil(check_every 16) stops there.  Then the timed windows ALTERNATE between three variants in one run:
the parent's TraceUntil, this tree's TraceUntil, this tree's TraceAdaptive, all from 0 spp to that target (a window = Reset, 32 frames of warm-up,
Reset, the timed call under a host clock).  Every variant's median and spread (min .. max over the repeats) are reported.  Last, the price of a
late pass: 16 more frames over the blocks the adaptive run left active, against 16 frames of the whole image."""
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
EVERY = 16


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

    def fresh():
        pt.Reset()
        pt.SetNoiseStats(True)
        pt.Trace(True, WARMUP)
        pt.Reset()

    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "probe":  # probe CAP -> the worst block's noise at every check of a uniform run
            fresh()
            out = []
            for _ in range(int(cmd[1]) // EVERY):
                pt.Trace(True, EVERY)
                out.append(pt.GetNoise()["worst_block"])
            print(" ".join(repr(v) for v in out), flush=True)
        elif cmd[0] == "until":  # until TARGET CAP -> ms, spp, sha1 of the image
            fresh()
            t0 = time.perf_counter()
            g = pt.TraceUntil(float(cmd[1]), EVERY, int(cmd[2]), EVERY)
            ms = (time.perf_counter() - t0) * 1e3
            print("%.4f %d %s" % (ms, g["spp"], hashlib.sha1(pt.ReadResult().tobytes()).hexdigest()), flush=True)
        elif cmd[0] == "adaptive":  # adaptive TARGET CAP -> ms, spp, frozen, blocks, pixel_samples, mean_noise, worst_block, sha1
            fresh()
            t0 = time.perf_counter()
            g = pt.TraceAdaptive(float(cmd[1]), EVERY, int(cmd[2]), EVERY)
            ms = (time.perf_counter() - t0) * 1e3
            print("%.4f %d %d %d %d %r %r %s" % (ms, g["spp"], g["blocks_frozen"], g["blocks"], g["pixel_samples"], g["mean_noise"], g["worst_block"],
                                               hashlib.sha1(pt.ReadResult().tobytes()).hexdigest()), flush=True)
        elif cmd[0] == "tail":  # tail TARGET CAP N -> after an adaptive run: active blocks, their pixels, median ms of N x 16 frames over them; then of the whole image
            fresh()
            g = pt.TraceAdaptive(float(cmd[1]), EVERY, int(cmd[2]), EVERY)
            idx, spp = pt.ReadBlockSPP()
            active = spp == pt.GetSPP()
            nbx = (width + 31) // 32
            px = sum(min(32, width - (int(b) % nbx) * 32) * min(32, height - (int(b) // nbx) * 32) for b in idx[active])
            ts = []
            for _ in range(int(cmd[3]) if px else 0):
                t0 = time.perf_counter()
                pt.Trace(True, EVERY)
                ts.append((time.perf_counter() - t0) * 1e3)
            pt.Reset()
            pt.Trace(True, WARMUP)
            tu = []
            for _ in range(int(cmd[3])):
                t0 = time.perf_counter()
                pt.Trace(True, EVERY)
                tu.append((time.perf_counter() - t0) * 1e3)
            print("%d %d %.4f %.4f" % (int(active.sum()), px, statistics.median(ts) if ts else 0.0, statistics.median(tu)), flush=True)
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
            raise SystemExit("adaptive_cost: a worker ended early (exit code %s)" % self.p.wait())  # nothing more is started on the GPU
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
    ap.add_argument("--stop-at", type=int, default=256, help="the spp at which the uniform TraceUntil is to stop (a multiple of 16 in [144, 496])")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_sampling.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.scene, args.width, args.height, args.cache)
    if not args.parent_tree:
        raise SystemExit("adaptive_cost: --parent-tree DIR (a built checkout of the parent commit) is needed")
    assert args.stop_at % EVERY == 0 and 128 < args.stop_at < 512
    os.makedirs(args.cache, exist_ok=True)
    cap = 512
    new = Worker(ROOT, args)
    old = Worker(os.path.abspath(args.parent_tree), args)
    variants = [("parent TraceUntil", old, "until"), ("TraceUntil", new, "until"), ("TraceAdaptive", new, "adaptive")]
    ms = {name: [] for name, _, _ in variants}
    last = {}
    try:
        wb = [float(v) for v in new.ask("probe %d" % cap)]
        k = args.stop_at // EVERY - 1
        assert min(wb[:k]) > wb[k], "the worst block's noise does not fall monotonically to the stop: choose another --stop-at"
        target = (min(wb[:k]) * wb[k]) ** 0.5
        for name, w, what in variants:  # one untimed window each: code objects loaded, buffers allocated once
            w.ask("%s %r %d" % (what, target, cap))
        for _ in range(args.repeats):
            for name, w, what in variants:
                a = w.ask("%s %r %d" % (what, target, cap))
                ms[name].append(float(a[0]))
                assert last.setdefault(name, a[1:]) == a[1:], "%s: two windows gave different results" % name
        tail = new.ask("tail %r %d 9" % (target, cap))
    finally:
        new.close()
        old.close()
    assert last["parent TraceUntil"] == last["TraceUntil"], "the uniform run differs from the parent's: %s" % last
    spp_u = int(last["TraceUntil"][0])
    assert spp_u == args.stop_at
    spp_a, frozen, blocks, samples = (int(v) for v in last["TraceAdaptive"][:4])
    pixels = args.width * args.height
    lines = ["Adaptive sampling: %s, %d x %d, %d bounces, tmpLifetime %d, %s frames in flight; target %.6g (worst block at %d / %d spp: %.6g / %.6g); check every %d, min %d, cap %d."
             % (args.scene, args.width, args.height, PT_CFG["maxBounce"], PT_CFG["tmpLifetime"], new.ready[2], target, args.stop_at - EVERY, args.stop_at, wb[k - 1], wb[k], EVERY, EVERY, cap),
             "A window = Reset, %d frames of warm-up, Reset, the call from 0 spp under a host clock; %d repeats, the three variants alternating in one run." % (WARMUP, args.repeats),
             "The uniform run stops at %d spp in both trees, images bit-identical (sha1 %s)." % (spp_u, last["TraceUntil"][1][:12]),
             "",
             "%-18s %10s %10s %10s %9s %7s %16s %14s" % ("variant", "median ms", "min ms", "max ms", "spread", "spp", "pixel-samples", "ms / Msample")]
    for name, _, what in variants:
        v = ms[name]
        med = statistics.median(v)
        n = samples if what == "adaptive" else spp_u * pixels
        lines.append("%-18s %10.2f %10.2f %10.2f %8.2f%% %7d %16d %14.4f" % (name, med, min(v), max(v), 100.0 * (max(v) - min(v)) / med, spp_a if what == "adaptive" else spp_u, n, med / (n * 1e-6)))
    po, pn = ms["parent TraceUntil"], statistics.median(ms["TraceUntil"])
    lines += ["",
              "this tree's TraceUntil median %.2f ms %s the parent's min .. max (%.2f .. %.2f ms)" % (pn, "lies inside" if min(po) <= pn <= max(po) else "lies OUTSIDE", min(po), max(po)),
              "TraceAdaptive: counter at %d spp, %d of %d blocks frozen, %d pixel-samples = %.1f %% of the %d x %d of a uniform run to its own counter, %.1f %% of the uniform TraceUntil's"
              % (spp_a, frozen, blocks, samples, 100.0 * samples / (spp_a * pixels), spp_a, pixels, 100.0 * samples / (spp_u * pixels)),
              "mean_noise %.6g worst_block %.6g afterwards" % (float(last["TraceAdaptive"][4]), float(last["TraceAdaptive"][5]))]
    n_active, px_active, t_active, t_whole = int(tail[0]), int(tail[1]), float(tail[2]), float(tail[3])
    if px_active:
        lines += ["a late pass: %d frames over the %d blocks still active (%d pixels): median %.3f ms = %.4f ms / Msample; over the whole image: %.3f ms = %.4f ms / Msample (9 calls each)"
                  % (EVERY, n_active, px_active, t_active, t_active / (EVERY * px_active * 1e-6), t_whole, t_whole / (EVERY * pixels * 1e-6))]
    else:
        lines += ["no block was left active at the end of the adaptive run; %d frames over the whole image: median %.3f ms" % (EVERY, t_whole)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
