"""What rectifying stale history costs in the temporal merge (Denoise(temporal=True, rectify=True)) next to the plain temporal call — DESIGN.md §4
"Rectifying stale history"; writes profiles/rectify_cost.txt.

    python tools/rectify_cost.py [--scene sponza] [--spp 4] [--repeats 5] [--out profiles/rectify_cost.txt]

One process, the scene at 1920 x 1080 with bench.py's settings.  A pose one camera step away (1.5 degrees of yaw, a seed of its own) is rendered and
committed, then the bench camera is rendered under a quarter of the sun, and `repeats` times, in turn, each after one untimed call of its kind, with
commit=False on the same inputs:
    Denoise(temporal=True)                                GetDenoiseMergeMs(): k_temporal_merge<false, false> — the yardstick: the call there was before
    Denoise(temporal=True, rectify=True, rectify_radius=R)  for R = 1, 2, 3: GetDenoiseMergeMs() (k_rectify_window<R> + k_temporal_merge<false, true>) and
                                                          GetDenoiseRectify()["window_ms"] (k_rectify_window<R> alone)
and of every call the time of its first a-trous level, for scale.  Beside them the byte model of the window kernel — the tile with its halo read once
(64 B per tile pixel) and 32 B written per pixel — and the registers, LDS bytes and scratch of the new kernel instances as the compiler reports them
(build/denoise.s, made here when it is missing).  A step that fails ends the run: nothing more is started on the GPU."""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.pose_cost import PT_CFG  # noqa: E402

CSRC = os.path.join(ROOT, "adypt_amd", "csrc")
GROUP_X, GROUP_Y = 32, 8  # the workgroup of k_rectify_window (kAtrousX, kAtrousY in denoise.hip)
DIM = 0.25


def row(name, v):
    return "%-60s %10.4f %10.4f %10.4f" % (name, statistics.median(v), min(v), max(v))


def kernel_resources():
    """[(demangled-ish name, vgprs, sgprs, LDS bytes, scratch bytes)] of the rectify instances in denoise.hip's code object"""
    asm = os.path.join(CSRC, "build", "denoise.s")
    if not os.path.exists(asm):
        subprocess.check_call(["make", "-C", CSRC, "build/denoise.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    out = []
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        lds, name, scratch, sgpr, vgpr = m.groups()
        w = re.search(r"k_rectify_windowILi(\d)E", name)
        g = re.search(r"k_temporal_mergeILb([01])ELb1E", name)
        if w:
            out.append(("k_rectify_window<%s>" % w.group(1), int(vgpr), int(sgpr), int(lds), int(scratch)))
        elif g:
            out.append(("k_temporal_merge<%s, true>" % ("true" if g.group(1) == "1" else "false"), int(vgpr), int(sgpr), int(lds), int(scratch)))
    return sorted(out)


def byte_model(width, height, radius):
    """bytes the window kernel moves: every workgroup reads its tile with the halo, clipped at the image border, 64 B per pixel, and writes 32 B per pixel"""
    read = 0
    for y0 in range(0, height, GROUP_Y):
        rows = min(y0 + GROUP_Y + radius, height) - max(y0 - radius, 0)
        for x0 in range(0, width, GROUP_X):
            read += rows * (min(x0 + GROUP_X + radius, width) - max(x0 - radius, 0)) * 64
    return read, 32 * width * height


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_cost.txt"))
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (its copy of the HIP runtime first, as bench.py does)
    except ImportError:
        pass
    from adypt_amd import api, scenes
    os.makedirs(args.cache, exist_ok=True)
    spec = scenes.make_scene(args.scene, args.cache, width=args.width, height=args.height, pt=PT_CFG)
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=12345), api.InstanceConfig.last_error()
    p, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    p.SetNoiseStats(True)
    for yaw, seed, sun in ((c.yaw + 1.5, 12346, 1.0), (c.yaw, 12345, DIM)):  # the earlier pose, committed; then the bench camera under the dimmed sun
        p.Reset()
        prm = cfg.pt_params(seed)
        prm.sun[:] = [v * sun for v in c.sun]
        p.SetConfig(prm)
        ip, iv = api.camera_matrices(c.fov, yaw, c.pitch, args.width, args.height)
        p.SetCamera(ip, iv, inst.m_camera.position)
        p.Trace(True, args.spp)
        if seed == 12346:
            p.Denoise(temporal=True)
    calls = [("plain", dict())] + [("radius %d" % r, dict(rectify=True, rectify_radius=r)) for r in (1, 2, 3)]
    merge, window, level = ({name: [] for name, _ in calls} for _ in range(3))
    for k in range(args.repeats + 1):
        for name, kw in calls:
            p.Denoise(temporal=True, commit=False, **kw)
            if k:
                merge[name].append(p.GetDenoiseMergeMs())
                level[name].append(p.GetDenoiseTiming()["levels"][0])
                if kw:
                    info = p.GetDenoiseRectify()
                    assert info["radius"] == kw["rectify_radius"]
                    window[name].append(info["window_ms"])
    kept, length, hit = p.ReadDenoiseRectify(), p.ReadDenoiseHistory(), p.ReadDenoiseGuides()["hit"]
    info = p.GetDenoiseRectify()
    p.destroy()

    px = args.width * args.height
    m_plain = statistics.median(merge["plain"])
    lines = ["Rectifying stale history in the temporal merge: %s, %d x %d, %d spp per pose, a pose 1.5 degrees of yaw away committed, the measured pose under %.2f of the sun;"
             % (args.scene, args.width, args.height, args.spp, DIM),
             "%d repeats, the four calls in turn in one run with commit=False on the same inputs.  HIP events." % args.repeats,
             "Radius 3: kept < 1 on %d of %d hit pixels, mean kept %.3f, mean history length on hit pixels %.2f." % (int((kept[hit] < 1).sum()), int(hit.sum()), float(kept[hit].mean()), float(length[hit].mean())),
             "On the device: %d bytes (36 per pixel = %d)." % (info["device_bytes"], 36 * px), "",
             "%-60s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"),
             row("Denoise(temporal=True): GetDenoiseMergeMs(), the yardstick", merge["plain"]),
             row("  its first a-trous level (k_atrous<false>, step 1)", level["plain"])]
    for r in (1, 2, 3):
        name = "radius %d" % r
        read, written = byte_model(args.width, args.height, r)
        m_merge, m_window = statistics.median(merge[name]), statistics.median(window[name])
        lines += ["", row("... rectify=True, radius %d: GetDenoiseMergeMs()" % r, merge[name]),
                  row("  of it k_rectify_window<%d> (window_ms)" % r, window[name]),
                  row("  its first a-trous level", level[name]),
                  "  merge stage / plain merge stage, medians: %.2f x; window / plain merge stage: %.2f x; window / one a-trous level: %.2f x"
                  % (m_merge / m_plain, m_window / m_plain, m_window / statistics.median(level[name])),
                  "  byte model of the window kernel: %d B read (%.1f per pixel: the tile and its halo once) + %d B written (32 per pixel) = %.1f MB -> %.2f TB/s at the median"
                  % (read, read / px, written, (read + written) / 1e6, (read + written) / (m_window * 1e-3) / 1e12),
                  "  taps: %d per pixel x 14 LDS words = %.1f G LDS words read -> %.1f T words/s at the median"
                  % ((2 * r + 1) ** 2, (2 * r + 1) ** 2 * 14 * px / 1e9, (2 * r + 1) ** 2 * 14 * px / (m_window * 1e-3) / 1e12)]
    lines += ["", "The new kernel instances (gfx950, as compiled):", "%-32s %6s %6s %10s %8s" % ("", "VGPRs", "SGPRs", "LDS bytes", "scratch")]
    lines += ["%-32s %6d %6d %10d %8d" % k for k in kernel_resources()]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
