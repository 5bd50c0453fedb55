"""What the trees a moved scene can get are worth, without a GPU: nodes visited and triangles tested per ray by the CPU oracle (DESIGN.md §4 "What the
tree is worth"; the figures go into profiles/rebuild_cost.txt by hand).

    python tools/tree_quality.py [--scene sponza] [--rays 200000] [--radii 8,16] [--split-budget 0.1,0.3]

The scene's triangles in the rest pose and in the wave pose of the tests (y += 1.5 sin(0.7 x) + 0.8 cos(0.9 z); x *= 1.1); random rays with origins
uniform in the pose's box and normal directions (tests/refit_truth.py rays_in_box), stack 64.  Trees: WideBVH.BuildLinear, WideBVH.BuildPLOC at every
radius (with the rounds it takes, counted by the numpy restatement tests/ploc_truth.py), at radius 8 with every --split-budget (large triangles split
first: csrc/device/presplit.hpp), WideBVH.Build (SBVH, the config's depth) of the pose."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--rays", type=int, default=200000)
    ap.add_argument("--radii", default="8,16")
    ap.add_argument("--split-budget", default="", help="comma-separated budgets of BuildPLOC(radius 8, split_budget)")
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    args = ap.parse_args()
    from adypt_amd import api, scenes
    from oracle import oracle_py as O
    from tests import ploc_truth
    from tests import refit_truth as T
    os.makedirs(args.cache, exist_ok=True)
    spec = scenes.make_scene(args.scene, args.cache)
    cfg = api.InstanceConfig()
    assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
    scene = api.Scene()
    assert scene.LoadFromFile(cfg.m_obj_filename)
    rest = np.array(scene.triangles).view(O.TRI_DT)
    print("%s: %d triangles, %d rays" % (args.scene, len(rest), args.rays))
    print("%-46s %8s %12s %13s %17s %9s" % ("", "nodes", "references", "nodes / ray", "triangles / ray", "build s"))
    for pose, tris in (("rest", rest), ("wave", T.wave(rest))):
        plain = api.Scene.FromArrays(tris, scene.materials)
        rays = T.rays_in_box(tris, args.rays)
        builders = [("linear tree (BuildLinear)", lambda b: b.BuildLinear(plain, cfg.bvh_params()))]
        for r in (int(x) for x in args.radii.split(",")):
            builders.append(("PLOC tree, radius %d (BuildPLOC)" % r, lambda b, r=r: b.BuildPLOC(plain, cfg.bvh_params(), r)))
        for budget in (float(x) for x in args.split_budget.split(",") if x):
            builders.append(("PLOC tree, radius 8, split budget %g" % budget, lambda b, budget=budget: b.BuildPLOC(plain, cfg.bvh_params(), 8, budget)))
        builders.append(("SBVH tree built for the pose (Build)", lambda b: b.Build(plain, cfg.bvh_params())))
        hits = {}
        for name, build in builders:
            b = api.WideBVH()
            t0 = time.perf_counter()
            build(b)
            s = time.perf_counter() - t0
            h = O.trace(O.Scene(b.nodes, b.tri_indices, tris, scene.materials), rays, stack_size=64)
            hits[name] = h
            print("%-5s %-40s %8d %12d %13.2f %17.2f %9.2f" % (pose, name, len(b.nodes) // 80, len(b.tri_indices), h["nodes"].mean(), h["tris"].mean(), s), flush=True)
        for r in (int(x) for x in args.radii.split(",")):
            print("      PLOC tree, radius %d: %d rounds" % (r, ploc_truth.tree(tris, r)[2]), flush=True)
        ref = hits[builders[-1][0]]
        for name, _ in builders[:-1]:
            h = hits[name]
            print("      %s against the SBVH tree: t differs on %d rays, tri_id on %d" % (name, (h["t"].view(np.uint32) != ref["t"].view(np.uint32)).sum(), (h["tri_id"] != ref["tri_id"]).sum()))


if __name__ == "__main__":
    main()
