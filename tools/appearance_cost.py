"""What changing the surfaces costs (SetMaterials, UpdateTexture, SetTriangleAttributes: csrc/device/appearance.hip) next to the only road there was
before: destroy the context and create it again with the new table — DESIGN.md §4 "Appearance"; writes profiles/appearance_cost.txt.

    python tools/appearance_cost.py [--scene sponza] [--repeats 6] [--parent-root DIR] [--out profiles/appearance_cost.txt]

One process, the scene at 1920 x 1080 with bench.py's settings, its first tree built on the GPU (PLOC, radius 8).  Five calls, `repeats` times,
alternating, each after one untimed call of its kind, with the host clock around the call and the HIP-event stages of GetAppearance():
  (a) SetMaterials(table): the table alone, the textures kept — two tables in turn, the emitters on and off
  (b) SetMaterials(table, textures): the table and all textures — two sets of texels in turn
  (c) UpdateTexture(0, rgb): the largest texture's texels in place
  (d) SetTriangleAttributes(0, ids): a material id for every triangle       (e) the same with texture coordinates
(d) is measured twice, the two in both orders: with k_ref_attributes (what ships) and on a second context created under ADYPT_APPEARANCE_EXPAND=1, which
re-expands the whole per-reference copy (ctx_expand_references) instead: the measurement the choice between the two rests on.
The road before, (f): a child process — with --parent-root importing adypt_amd from that directory, a built checkout of the parent commit — creates the context once, reads
its tree, Woop data and indices back, and then times adypt_destroy + adypt_create with those arrays and the new table: the cheapest recreate there is,
no tree built and no Woop data computed.  What it cannot keep — the denoiser's history, bindings, the tree-cost reference — is not priced.
A step that fails ends the run: nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pose_cost import PT_CFG, TRI_DT, table  # noqa: E402

APPEARANCE_STAGES = ("staged_ms", "packed_ms", "classified_ms")


def load(args):
    try:
        import torch  # noqa: F401  (its copy of the HIP runtime first, as bench.py does)
    except ImportError:
        pass
    if args.package_root:
        sys.path.insert(0, os.path.abspath(args.package_root))
    from adypt_amd import api, scenes
    os.makedirs(args.cache, exist_ok=True)
    spec = scenes.make_scene(args.scene, args.cache, width=args.width, height=args.height, pt=PT_CFG)
    cfg = api.InstanceConfig()
    assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
    scene = api.Scene()
    assert scene.LoadFromFile(cfg.m_obj_filename)
    cam = api.Camera()
    cam.Initialize(cfg, cfg.m_width, cfg.m_height)
    return api, cfg, scene, cam


def first_tracer(api, cfg, scene, cam):
    hs = api.HipScene()
    hs.Initialize(scene, None)
    p = api.HipPathTracer()
    p.Initialize(cfg.pt_params(12345), hs, cfg.m_width, cfg.m_height, cfg=cfg.bvh_params(), method="ploc", radius=8)
    ip, iv = cam.matrices()
    p.SetCamera(ip, iv, cam.position)
    return p


def recreate_child(args):
    """(f): destroy + create with the tree, Woop data and indices read back from a first context; prints one JSON line"""
    api, cfg, scene, cam = load(args)
    p = first_tracer(api, cfg, scene, cam)
    nodes, woop = p.ReadBVH()
    b = api.WideBVH()
    b.nodes, b.tri_indices = nodes, p.ReadTriIndices()
    hs = api.HipScene()
    hs.Initialize(scene, b, woop)
    ip, iv = cam.matrices()
    ms = []
    for k in range(args.repeats + 1):
        t0 = time.perf_counter()
        p.destroy()
        p = api.HipPathTracer()
        p.Initialize(cfg.pt_params(12345), hs, cfg.m_width, cfg.m_height)
        p.SetCamera(ip, iv, cam.position)
        p.DeviceSynchronize()
        if k:  # (the first is untimed)
            ms.append((time.perf_counter() - t0) * 1e3)
    p.Trace(True, 1)  # (the context works)
    p.destroy()
    print("RECREATE " + json.dumps({"ms": ms, "package": os.path.dirname(os.path.abspath(api.__file__))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--cache", default=os.environ.get("ADYPT_CACHE") or os.path.join(ROOT, ".adypt_cache"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "appearance_cost.txt"))
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit: the recreate road is measured with its adypt_amd")
    ap.add_argument("--recreate-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--package-root", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.recreate_child:
        return recreate_child(args)
    api, cfg, scene, cam = load(args)
    O_MAT = np.dtype([("dtex", "<i4"), ("kd", "<f4", 3), ("etex", "<i4"), ("ke", "<f4", 3), ("stex", "<i4"), ("ks", "<f4", 3), ("illum", "<i4"), ("shininess", "<f4"),
                      ("dissolve", "<f4"), ("ior", "<f4")])
    tris = np.array(scene.triangles).view(TRI_DT)
    n = len(tris)
    mats = np.array(scene.materials).view(O_MAT)
    off = mats.copy()
    off["ke"] = 0.0
    gloss = mats.copy()  # (another class for every diffuse material: every class word of theirs flips)
    gloss["illum"], gloss["shininess"] = np.where(mats["illum"] == 1, 2, mats["illum"]), np.where(mats["illum"] == 1, 200.0, mats["shininess"])
    tex = [np.array(t) for t in scene.textures]
    tex2 = [np.ascontiguousarray(255 - t) for t in tex]
    largest = int(np.argmax([t.size for t in tex])) if tex else -1
    texels = sum(t.shape[0] * t.shape[1] for t in tex)
    ids = [np.ascontiguousarray(tris["matid"]), np.ascontiguousarray((tris["matid"] + 1) % max(1, len(mats)), dtype=np.int32)]
    uv = [np.ascontiguousarray(tris["tc"].reshape(-1, 6)), np.ascontiguousarray(tris["tc"].reshape(-1, 6) * np.float32(0.5))]
    p = first_tracer(api, cfg, scene, cam)
    n_nodes, n_refs = p.GetBVHSizes()

    def timed(call):
        t0 = time.perf_counter()
        info = call()
        ms = (time.perf_counter() - t0) * 1e3  # (every setter ends in a stream synchronise)
        return [ms] + [info[k] for k in APPEARANCE_STAGES] + [info["reclassed"]]

    os.environ["ADYPT_APPEARANCE_EXPAND"] = "1"  # (read when a context is created)
    whole = first_tracer(api, cfg, scene, cam)
    del os.environ["ADYPT_APPEARANCE_EXPAND"]
    routes = [("(a) SetMaterials(table), textures kept", lambda k: p.SetMaterials((off, gloss)[k % 2])),
              ("(b) SetMaterials(table, textures)", lambda k: p.SetMaterials((off, gloss)[k % 2], (tex, tex2)[k % 2]))]
    if tex:
        routes.append(("(c) UpdateTexture(%d): %d x %d" % (largest, tex[largest].shape[1], tex[largest].shape[0]), lambda k: p.UpdateTexture(largest, (tex, tex2)[k % 2][largest])))
    routes += [("(d) SetTriangleAttributes(ids), k_ref_attributes", lambda k: p.SetTriangleAttributes(0, ids[k % 2])),
               ("(d') the same, whole copy re-expanded", lambda k: whole.SetTriangleAttributes(0, ids[k % 2])),
               ("(e) SetTriangleAttributes(ids, texcoords)", lambda k: p.SetTriangleAttributes(0, ids[k % 2], uv[k % 2]))]
    rows = {name: [] for name, _ in routes}
    for name, call in routes:
        call(1)  # untimed: staging buffers, code objects
    for k in range(args.repeats):
        order = list(routes)
        if k % 2:  # (d) and (d') in both orders: whichever runs second finds the records in the cache
            i = [name[:4] for name, _ in order].index("(d) ")
            order[i], order[i + 1] = order[i + 1], order[i]
        for name, call in order:
            rows[name].append(timed(lambda: call(k)))
    # the state after all of it is the state of a context created from the same arrays
    p.SetMaterials(mats, tex)
    p.SetTriangleAttributes(0, ids[0], uv[0])
    want = api.pack_appearance(mats, tex)
    assert p.ReadMaterialRecords().tobytes() == want[0].tobytes() and p.ReadTexels().tobytes() == want[1].tobytes(), "the device's table and arena are not adypt_pack_appearance's"
    assert p.ReadTriangles().tobytes() == np.ascontiguousarray(scene.triangles).tobytes(), "the records do not unpack to the scene's triangles"
    info = p.GetAppearance()
    p.Trace(True, 1)
    p.destroy()
    whole.destroy()
    # (f) in a process of its own, after this one has let go of the device
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--recreate-child", "--scene", args.scene, "--width", str(args.width), "--height", str(args.height),
                            "--repeats", str(args.repeats), "--cache", args.cache] + (["--package-root", args.parent_root] if args.parent_root else []),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    found = [line for line in child.stdout.decode().splitlines() if line.startswith("RECREATE ")]
    assert child.returncode == 0 and found, child.stdout.decode()[-3000:]
    recreate = json.loads(found[0][len("RECREATE "):])["ms"]

    lines = ["Cost of changing the surfaces: %s (%d triangles, %d references, %d materials, %d textures of %d texels together), %d x %d, %d bounces, PLOC tree built on the GPU; "
             "%d repeats, the calls alternating in one run." % (args.scene, n, n_refs, len(mats), len(tex), texels, args.width, args.height, PT_CFG["maxBounce"], args.repeats),
             "The byte model: a texel is 3 B up and 4 B written (all textures: %d B up, %d B written); a reclassified triangle is 8 B read and 8 B written (%d B each way), with texture "
             "coordinates 24 B up and 24 B more written; k_ref_attributes reads 4 B and, in the range, moves 48 B per reference (%d B read and written); the whole copy re-expanded is "
             "128 B read and written per reference (%d B)." % (3 * texels, 4 * (texels + sum(t.shape[0] for t in tex)), 8 * n, 48 * n_refs, 128 * n_refs),
             "Table, arena and staging buffers hold %d bytes on the device.  Afterwards the table and the arena equal adypt_pack_appearance's and the records unpack to the scene's "
             "triangles, byte for byte." % info["device_bytes"], ""]
    for name, _ in routes:
        v = rows[name]
        lines += table("%s (the first row is the host clock around the call; the others HIP events, GetAppearance(); reclassed %d):" % (name, v[-1][4]),
                       [("host clock", [r[0] for r in v]), ("staged: the copies from the host", [r[1] for r in v]), ("packed: k_pack_texels", [r[2] for r in v]),
                        ("classified: k_tri_attributes + references", [r[3] for r in v])]) + [""]
    lines += table("(f) the road before: adypt_destroy + adypt_create with the tree, Woop data and indices at hand (host clock, a process of its own, %s):" % (
        "the parent commit's build" if args.parent_root else "THIS build: no --parent-root was given"), [("host clock", recreate)]) + [""]
    med = {name[:4].strip(): statistics.median(r[0] for r in rows[name]) for name, _ in routes}
    f_ms = statistics.median(recreate)
    lines.append("Measured, medians, host clock: " + "   ".join("%s %.3f ms" % (k, v) for k, v in med.items()) + "   (f) %.3f ms: (f) / (b) = %.1f, (f) / (a) = %.1f" % (
        f_ms, f_ms / med["(b)"], f_ms / med["(a)"]))
    cls = {name[:4].strip(): statistics.median(r[3] for r in rows[name]) for name, _ in routes}
    lines.append("The per-reference copy, medians of the classified stage of (d): k_ref_attributes %.3f ms, whole copy re-expanded %.3f ms: ratio %.2f" % (
        cls["(d)"], cls["(d')"], cls["(d')"] / cls["(d)"] if cls["(d)"] else float("nan")))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
