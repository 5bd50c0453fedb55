"""What following mirrors and glass costs in the denoiser (Denoise(specular_bounces=K)) next to the plain call — DESIGN.md §4 "Guides through mirrors and
glass"; writes profiles/specular_cost.txt.

    python tools/specular_cost.py [--scene sponza] [--spp 64] [--repeats 7] [--out profiles/specular_cost.txt]

One process, the scene at 1920 x 1080 with bench.py's settings, --spp samples once.  Then `repeats` times, in turn, each after one untimed call of its
kind, on the same image:
    Denoise()                      GetDenoiseTiming(): "guides" is the guide capture alone — the yardstick the chain is held against — and "total"
    Denoise(specular_bounces=K)    for K = 1, 4, 8: GetDenoiseSpecular()["chain_ms"] (k_chain_start + K rounds of k_trace and k_chain_step, HIP events), its
                                   rays and pixel counts, and GetDenoiseTiming()["total"], whose "guides" stage holds the capture and the chain
Beside them the registers and scratch of the new kernels as the compiler reports them (build/denoise.s, made here when it is missing).  A step that
fails ends the run: nothing more is started on the GPU."""
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
BOUNCES = (1, 4, 8)


def row(name, v):
    return "%-72s %10.4f %10.4f %10.4f" % (name, statistics.median(v), min(v), max(v))


def kernel_resources():
    asm = os.path.join(CSRC, "build", "denoise.s")
    if not os.path.exists(asm):
        subprocess.check_call(["make", "-C", CSRC, "build/denoise.s"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    out = []
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        name, scratch, sgpr, vgpr = m.groups()
        short = re.search(r"(k_chain_start|k_chain_step|k_denoise_prepare_class|k_denoise_prepare)(?:ILb0E)?E", name)  # (the chain's kernels: the instances that do not unfold)
        if short:
            out.append((short.group(1), int(vgpr), int(sgpr), int(scratch)))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specular_cost.txt"))
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
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    p.Trace(True, args.spp)
    calls = [(0, dict())] + [(k, dict(specular_bounces=k)) for k in BOUNCES]
    guides, total, chain, info = ({k: [] for k, _ in calls} for _ in range(4))
    for r in range(args.repeats + 1):
        for k, kw in calls:
            p.Denoise(**kw)
            if not r:
                continue
            t = p.GetDenoiseTiming()
            guides[k].append(t["guides"])
            total[k].append(t["total"])
            if k:
                i = p.GetDenoiseSpecular()
                assert i["bounces"] == k
                chain[k].append(i["chain_ms"])
                info[k] = i
    hit = p.ReadDenoiseGuides()["hit"]
    p.destroy()

    px = args.width * args.height
    capture = statistics.median(guides[0])
    lines = ["Guides through mirrors and glass: %s, %d x %d, %d spp; %d repeats, the four calls in turn in one run on the same image.  HIP events." % (args.scene, args.width, args.height, args.spp, args.repeats),
             "%d of %d pixels hit; the capture traces 3 rays per pixel = %d." % (int(hit.sum()), px, 3 * px), "",
             "%-72s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"),
             row("Denoise(): the guide capture (three viewer launches), the yardstick", guides[0]),
             row("  the whole call (capture, prepare, 5 levels)", total[0])]
    for k in BOUNCES:
        i = info[k]
        m = statistics.median(chain[k])
        lines += ["", row("Denoise(specular_bounces=%d): chain_ms" % k, chain[k]),
                  row("  its guides stage (capture + chain)", guides[k]),
                  row("  the whole call", total[k]),
                  "  rays %d (%.3f of the capture's), followed %d, escaped %d, truncated %d pixels; device bytes %d (32 per local pixel + counters)"
                  % (i["rays"], i["rays"] / (3.0 * px), i["pixels_followed"], i["pixels_escaped"], i["pixels_truncated"], i["device_bytes"]),
                  "  chain / capture, medians: %.2f x; whole call / plain whole call: %.3f x; %d launches (1 + 2 per round: every round is enqueued, none is read back)"
                  % (m / capture, statistics.median(total[k]) / statistics.median(total[0]), 1 + 2 * k)]
    lines += ["", "The kernels (gfx950, as compiled):", "%-32s %6s %6s %8s" % ("", "VGPRs", "SGPRs", "scratch")]
    lines += ["%-32s %6d %6d %8d" % k for k in kernel_resources()]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
