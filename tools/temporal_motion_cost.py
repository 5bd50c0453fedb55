"""What following moved geometry costs in the temporal merge (Denoise(temporal=True, follow_motion=True)) next to the plain temporal call, and what the
snapshot copy of a committing call costs next to a device-to-device copy of the same bytes — DESIGN.md §4 "Following moved geometry"; writes
profiles/temporal_motion_cost.txt.

    python tools/temporal_motion_cost.py [--scene sponza] [--parts 16] [--spp 4] [--repeats 5] [--out profiles/temporal_motion_cost.txt]

One process, the scene at 1920 x 1080 with bench.py's settings, its first tree built on the GPU (PLOC, radius 8), cut into `parts` slabs as
tools/pose_cost.py cuts it.  Pose A is rendered and committed with follow_motion; then pose B — every triangle of the scene has moved — is rendered, and
  1. `repeats` times, alternating, each after one untimed call of its kind, with commit=False on the same inputs:
       Denoise(temporal=True)                      GetDenoiseMergeMs(): k_temporal_merge<false>, which is the kernel there was before follow_motion
                                                   existed, instruction for instruction
       Denoise(temporal=True, follow_motion=True)  GetDenoiseMergeMs(): k_motion_gather + k_temporal_merge<true>
  2. `repeats` committing motion calls after an untimed one: GetDenoiseMotion()["snapshot_ms"], the HIP-event time of k_motion_snapshot, next to
     HIP-event times of a device-to-device copy of as many bytes (torch, the same process).
A step that fails ends the run: nothing more is started on the GPU."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.pose_cost import PT_CFG, TRI_DT, slab_poses  # noqa: E402

MERGE_BOUND, SNAPSHOT_BOUND = 3.5, 1.5  # of the plain merge stage; of the device-to-device copy


def row(name, v):
    return "%-52s %10.4f %10.4f %10.4f" % (name, statistics.median(v), min(v), max(v))


def device_copy_ms(n_bytes, repeats):
    """HIP-event times of `repeats` device-to-device copies of n_bytes after an untimed one; None without torch"""
    try:
        import torch
    except ImportError:
        return None
    a = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    out = []
    for k in range(repeats + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        b.copy_(a)
        t1.record()
        torch.cuda.synchronize()
        if k:
            out.append(t0.elapsed_time(t1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parts", type=int, default=16)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_motion_cost.txt"))
    args = ap.parse_args()
    try:
        import torch  # noqa: F401  (its copy of the HIP runtime first, as bench.py does)
    except ImportError:
        pass
    from adypt_amd import api, scenes
    os.makedirs(args.cache, exist_ok=True)
    spec = scenes.make_scene(args.scene, args.cache, width=args.width, height=args.height, pt=PT_CFG)
    cfg = api.InstanceConfig()
    assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
    scene = api.Scene()
    assert scene.LoadFromFile(cfg.m_obj_filename)
    rest = np.array(scene.triangles).view(TRI_DT)
    n = len(rest)
    parts, sets = slab_poses(rest, args.parts)
    cam = api.Camera()
    cam.Initialize(cfg, cfg.m_width, cfg.m_height)
    ip, iv = cam.matrices()
    hs = api.HipScene()
    hs.Initialize(scene, None)
    p = api.HipPathTracer()
    p.Initialize(cfg.pt_params(12345), hs, cfg.m_width, cfg.m_height, cfg=cfg.bvh_params(), method="ploc", radius=8)
    p.SetCamera(ip, iv, cam.position)
    p.SetNoiseStats(True)
    p.BindParts(parts, args.parts)

    def render(k):
        p.Pose(sets[k])
        p.SetConfig(cfg.pt_params(12345 + k))  # (a seed per pose: README, History across poses)
        p.Trace(True, args.spp)

    render(0)
    p.Denoise(temporal=True, follow_motion=True)
    render(1)
    calls = (("plain", dict()), ("motion", dict(follow_motion=True)))
    merge = {name: [] for name, _ in calls}
    for k in range(args.repeats + 1):
        for name, kw in calls:
            p.Denoise(temporal=True, commit=False, **kw)
            if k:
                merge[name].append(p.GetDenoiseMergeMs())
    length, motion = p.ReadDenoiseHistory(), p.ReadDenoiseMotion()
    hit = p.ReadDenoiseGuides()["hit"]
    moved = motion["moved"]
    snapshot = []
    for k in range(args.repeats + 1):
        p.Denoise(temporal=True, follow_motion=True)
        if k:
            snapshot.append(p.GetDenoiseMotion()["snapshot_ms"])
    info = p.GetDenoiseMotion()
    p.destroy()
    copy = device_copy_ms(80 * n, args.repeats)

    px = args.width * args.height
    m_plain, m_motion = statistics.median(merge["plain"]), statistics.median(merge["motion"])
    lines = ["Following moved geometry in the temporal merge: %s (%d triangles), %d x %d, %d spp per pose, a whole-scene pose of %d parts between the committed pose and the measured one;"
             % (args.scene, n, args.width, args.height, args.spp, args.parts),
             "%d repeats, the two calls alternating in one run with commit=False on the same inputs.  HIP events." % args.repeats,
             "Moved: %d of %d hit pixels; %.1f %% of the moved pixels found history, mean history length on hit pixels %.2f."
             % (int(moved.sum()), int(hit.sum()), 100.0 * float((length[moved] > args.spp).mean()) if moved.any() else 0.0, float(length[hit].mean())),
             "On the device: %d bytes (80 per triangle + 32 per pixel = %d)." % (info["device_bytes"], 80 * n + 32 * px), "",
             "The merge stage, GetDenoiseMergeMs():", "%-52s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"),
             row("Denoise(temporal=True): k_temporal_merge<false>", merge["plain"]),
             row("... follow_motion=True: gather + k_temporal_merge<true>", merge["motion"]),
             "motion / plain, medians: %.2f x (the byte model says about 2.5 x; accepted up to %.1f x): %s" % (m_motion / m_plain, MERGE_BOUND, "within" if m_motion <= MERGE_BOUND * m_plain else "EXCEEDED"),
             "", "The snapshot of a committing motion call, %d bytes:" % (80 * n), "%-52s %10s %10s %10s" % ("", "median ms", "min ms", "max ms"),
             row("k_motion_snapshot (GetDenoiseMotion()['snapshot_ms'])", snapshot)]
    if copy is None:
        lines.append("device-to-device copy of as many bytes: not measured (no torch)")
    else:
        m_snap, m_copy = statistics.median(snapshot), statistics.median(copy)
        lines += [row("device-to-device copy of as many bytes (torch)", copy),
                  "snapshot / copy, medians: %.2f x (accepted up to %.1f x): %s" % (m_snap / m_copy, SNAPSHOT_BOUND, "within" if m_snap <= SNAPSHOT_BOUND * m_copy else "EXCEEDED")]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
