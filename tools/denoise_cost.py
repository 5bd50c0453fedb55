"""What the denoiser costs, and that it costs nothing when unused (DESIGN.md §4 "Denoising"; writes profiles/denoise_cost.txt).

    python tools/denoise_cost.py --parent-tree DIR [--spp 64] [--steps 256] [--repeats 7] [--out profiles/denoise_cost.txt]

DIR is a built checkout of the parent commit (its own adypt_amd package and libadypt_hip.so).  Two worker processes hold one context each — the
parent's library and this tree's — on the bench scene at 1920 x 1080, 8 bounces.
  1. This tree, the noise statistics on, `spp` frames: `repeats` times Denoise() with the default parameters, the HIP-event times of the guide capture,
     of prepare and of every level (adypt_get_denoise_timing) and the host clock around the whole call (which includes the read-back of the result);
     one 1-spp step of the same run for scale; the 80 B per pixel a level must read and write against the time it took.
  2. Unused: the timed windows of Trace(True, steps) ALTERNATE between the parent and this tree (statistics off, Denoise() never called), as
     tools/noise_cost.py does; this tree's median is to lie inside the parent's own min .. max spread.  Both are written down.
  3. The temporal merge (this tree): a pose one camera step away (1.5 degrees of yaw, a seed of its own) is rendered and committed, then the bench
     camera again: `repeats` times Denoise(temporal=True, commit=False), the HIP-event time of k_temporal_merge (adypt_get_denoise_merge_ms), the
     164 B per pixel it moves against that time, and how many pixels found history.
  4. Denoise() without `temporal`, the two trees ALTERNATING in one run, the results bit-identical: the host clock around the call and the device
     total of its events; this tree's medians are to lie inside the parent's own spread, as in 2."""
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
        if cmd[0] == "window":  # window STEPS -> ms of the timed frames, sha1 of the image (statistics off, nothing denoised)
            pt.Reset()
            pt.Trace(True, WARMUP)
            t0 = time.perf_counter()
            pt.Trace(True, int(cmd[1]))
            ms = (time.perf_counter() - t0) * 1e3
            print("%.4f %s" % (ms, hashlib.sha1(pt.ReadResult().tobytes()).hexdigest()), flush=True)
        elif cmd[0] == "denoise":  # denoise SPP REPEATS -> per repeat: host ms, guides, prepare, the levels; then the ms of one 1-spp step
            pt.Reset()
            pt.SetNoiseStats(True)
            pt.Trace(True, int(cmd[1]))
            pt.Denoise()  # untimed: the images are allocated, the code object loaded
            rows = []
            for _ in range(int(cmd[2])):
                t0 = time.perf_counter()
                pt.Denoise()
                host = (time.perf_counter() - t0) * 1e3
                t = pt.GetDenoiseTiming()
                rows.append([host, t["guides"], t["prepare"]] + t["levels"])
            steps = []
            for _ in range(int(cmd[2])):
                t0 = time.perf_counter()
                pt.Trace(True, 1)
                steps.append((time.perf_counter() - t0) * 1e3)
            print(" ".join("%.4f" % v for r in rows for v in r) + " | " + " ".join("%.4f" % v for v in steps), flush=True)
            pt.Reset()
            pt.SetNoiseStats(False)
        elif cmd[0] == "temporal":  # temporal SPP REPEATS -> the merge's ms per repeat | hit pixels, hit pixels with history, mean length
            import numpy as np
            c, cfg, spp = inst.m_config.c, inst.m_config, int(cmd[1])
            pt.Reset()
            pt.SetNoiseStats(True)
            for yaw, seed in ((c.yaw + 1.5, 12346), (c.yaw, 12345)):  # the earlier pose, committed; then the bench camera
                pt.Reset()
                pt.SetConfig(cfg.pt_params(seed))
                ip, iv = api.camera_matrices(c.fov, yaw, c.pitch, width, height)
                pt.SetCamera(ip, iv, inst.m_camera.position)
                pt.Trace(True, spp)
                if seed == 12346:
                    pt.Denoise(temporal=True)
            rows = []
            for _ in range(int(cmd[2])):
                pt.Denoise(temporal=True, commit=False)
                rows.append(pt.GetDenoiseMergeMs())
            n, hit = pt.ReadDenoiseHistory(), pt.ReadDenoiseGuides()["hit"]
            print(" ".join("%.4f" % v for v in rows) + " | %d %d %.3f" % (int(hit.sum()), int((n[hit] > spp).sum()), float(n[hit].mean())), flush=True)
            pt.ResetDenoiseHistory()
            pt.Reset()
            pt.SetNoiseStats(False)
        elif cmd[0] == "plain_setup":  # plain_setup SPP: the state the plain windows filter
            pt.Reset()
            pt.SetNoiseStats(True)
            pt.Trace(True, int(cmd[1]))
            pt.Denoise()  # untimed
            print("ok", flush=True)
        elif cmd[0] == "plain":  # plain -> host ms of one Denoise(), the device total of its events, its guide capture, prepare + levels; sha1 of the result
            t0 = time.perf_counter()
            out = pt.Denoise()
            host = (time.perf_counter() - t0) * 1e3
            t = pt.GetDenoiseTiming()
            print("%.4f %.4f %.4f %.4f %s" % (host, t["total"], t["guides"], t["prepare"] + sum(t["levels"]), hashlib.sha1(out.tobytes()).hexdigest()), flush=True)
        elif cmd[0] == "plain_done":
            pt.Reset()
            pt.SetNoiseStats(False)
            print("ok", flush=True)
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
            raise SystemExit("denoise_cost: a worker ended early (exit code %s)" % self.p.wait())  # nothing more is started on the GPU
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
        return "BELOW the parent's own min .. max spread (faster than every window of the parent)"
    return "INSIDE the parent's own min .. max spread" if median <= max(parent) else "ABOVE the parent's own min .. max spread (slower than every window of the parent)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", metavar="TREE")
    ap.add_argument("--parent-tree")
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_cost.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.scene, args.width, args.height, args.cache)
    if not args.parent_tree:
        raise SystemExit("denoise_cost: --parent-tree DIR (a built checkout of the parent commit) is needed")
    os.makedirs(args.cache, exist_ok=True)
    new = Worker(ROOT, args)
    old = Worker(os.path.abspath(args.parent_tree), args)
    variants = [("parent commit", old), ("this tree, unused", new)]
    ms = {name: [] for name, _ in variants}
    plain = {name: [] for name, _ in variants}
    sha, plain_sha = {}, {}
    try:
        answer = new.ask("denoise %d %d" % (args.spp, args.repeats))
        old.ask("denoise %d %d" % (args.spp, args.repeats))  # (not reported: so that both contexts have the same history of calls and allocations from here on)
        for name, w in variants:
            w.ask("plain_setup %d" % args.spp)
        for k in range(args.repeats):
            for name, w in (variants if k % 2 == 0 else variants[::-1]):  # (who goes first alternates too)
                host, dev, guides, filt, h = w.ask("plain")
                plain[name].append((float(host), float(dev), float(guides), float(filt)))
                assert plain_sha.setdefault(name, h) == h, "%s: two Denoise() calls gave different images" % name
        assert len(set(plain_sha.values())) == 1, "the two trees do not denoise to the same image: %s" % plain_sha
        for name, w in variants:
            w.ask("plain_done")
        for name, w in variants:  # one untimed window each
            w.ask("window 64")
        for _ in range(args.repeats):
            for name, w in variants:
                t, h = w.ask("window %d" % args.steps)
                ms[name].append(float(t))
                assert sha.setdefault(name, h) == h, "%s: two windows gave different images" % name
        assert len(set(sha.values())) == 1, "the two trees do not render the same image: %s" % sha
        merge = new.ask("temporal %d %d" % (args.spp, args.repeats))  # last: until here this tree's context has never made a temporal call
    finally:
        new.close()
        old.close()
    bar = answer.index("|")
    flat, steps = [float(v) for v in answer[:bar]], [float(v) for v in answer[bar + 1:]]
    per = len(flat) // args.repeats
    rows = [flat[i * per:(i + 1) * per] for i in range(args.repeats)]
    levels = per - 3
    med = [statistics.median(r[k] for r in rows) for k in range(per)]
    lo = [min(r[k] for r in rows) for k in range(per)]
    hi = [max(r[k] for r in rows) for k in range(per)]
    px = args.width * args.height
    names = ["host clock, with read-back", "guide capture (3 launches)", "prepare"] + ["level %d (step %d)" % (l, 1 << l) for l in range(levels)]
    lines = ["Cost of Denoise(): %s, %d x %d, %d bounces, %d spp with the noise statistics on, default parameters (%d levels); %d repeats.  HIP-event times except the first row."
             % (args.scene, args.width, args.height, PT_CFG["maxBounce"], args.spp, levels, args.repeats),
             "",
             "%-28s %10s %10s %10s %12s" % ("", "median ms", "min ms", "max ms", "GB/s @ 80 B")]
    for k in range(per):
        gbs = ""
        if k >= 3:  # what a level moves at the least: the five float4 images once, 80 B per pixel (X0 read and written, X1, X2 read; XA by the last level only)
            gbs = "%12.0f" % (px * 80 / (med[k] * 1e-3) / 1e9)
        lines.append("%-28s %10.3f %10.3f %10.3f %s" % (names[k], med[k], lo[k], hi[k], gbs))
    lines += ["%-28s %10.3f" % ("device total (events)", sum(med[1:])),
              "one 1-spp step of the same run (host clock around Trace(True, 1)): median %.3f ms (min %.3f, max %.3f)" % (statistics.median(steps), min(steps), max(steps)),
              "a level is priced at %.1f MB: 80 B per pixel, the five float4 images once each" % (px * 80 / 1e6),
              "",
              "Unused (statistics off, Denoise() never called): window = %d warm-up + %d timed frames, host clock around Trace(True, %d); the two trees alternating in one run; images bit-identical (sha1 %s)."
              % (WARMUP, args.steps, args.steps, next(iter(sha.values()))[:12]),
              "%-20s %10s %10s %10s" % ("", "median ms", "min ms", "max ms")]
    for name, _ in variants:
        v = ms[name]
        lines.append("%-20s %10.2f %10.2f %10.2f" % (name, statistics.median(v), min(v), max(v)))
    p, n = ms["parent commit"], statistics.median(ms["this tree, unused"])
    lines.append("this tree's median lies %s" % verdict(p, n))
    bar = merge.index("|")
    mm, (hits, found, length) = [float(v) for v in merge[:bar]], merge[bar + 1:]
    m_med = statistics.median(mm)
    lines += ["",
              "Temporal merge (k_temporal_merge, HIP events): a pose 1.5 degrees of yaw away committed at %d spp, then the bench camera, Denoise(temporal=True, commit=False) %d times;"
              % (args.spp, args.repeats),
              "history on %s of %s hit pixels, mean length %s." % (found, hits, length),
              "%-28s %10s %10s %10s %12s" % ("", "median ms", "min ms", "max ms", "GB/s @ 164 B"),
              "%-28s %10.3f %10.3f %10.3f %12.0f" % ("merge", m_med, min(mm), max(mm), px * 164 / (m_med * 1e-3) / 1e9),
              "the merge is priced at %.1f MB: 164 B per pixel (64 B of the call's images and 64 B of history read, 36 B written; taps shared by neighbours counted once)" % (px * 164 / 1e6),
              "",
              "Denoise() without temporal at %d spp: the two trees alternating in one run, %d calls each; results bit-identical (sha1 %s)." % (args.spp, args.repeats, next(iter(plain_sha.values()))[:12]),
              "guide capture: the three launches of tracer.hip's camera kernel (its code object is the parent's byte for byte); prepare + levels: denoise.hip's own kernels.",
              "%-20s %-26s %10s %10s %10s" % ("", "", "median ms", "min ms", "max ms")]
    parts = ((0, "host clock, with read-back"), (1, "device total (events)"), (2, "guide capture"), (3, "prepare + levels"))
    for name, _ in variants:
        for k, what in parts:
            v = [r[k] for r in plain[name]]
            lines.append("%-20s %-26s %10.3f %10.3f %10.3f" % (name, what, statistics.median(v), min(v), max(v)))
    for k, what in parts:
        p, n = [v[k] for v in plain["parent commit"]], statistics.median(v[k] for v in plain["this tree, unused"])
        lines.append("%s: this tree's median lies %s" % (what, verdict(p, n)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
