"""The scenes of the geometry tests at scale (not a test module): a soup with two triangles far outside it, at counts just past the sizes at which
csrc/device/build.hip and rocPRIM's sort start to run other code.
    65 538      the partial boxes of k_centroid_box number 257: the one-workgroup second pass (stride 256) reaches the last one, which holds both
                outliers, only in its second round
    262 146     the first pass is capped at 1 024 workgroups of 256: elements 262 144 and 262 145, the outliers, are the second round of threads 0 and 1
                of workgroup 0
    1 048 578   two past rocprim::radix_sort_keys's merge_sort_limit (Onesweep from there on); the last workgroup of k_pose and the last group of
                k_motion_snapshot are ragged
The outliers are the extremes of the centroid box (and of the scene box) on every face, so a reduction that loses them makes other keys — another tree."""
import os
import re
import shutil

import numpy as np

from adypt_amd import api
from tests import refit_truth as T

COUNTS = (65538, 262146, 1048578)
FAR = 15.0          # the soup's centres lie in [-10, 10]^3, its vertices a few sigma of 0.3 around them
SPLIT_BUDGET = 0.3
_scenes, _trees = {}, {}


def far_ends(n):
    """refit_truth.soup(n, 11) with triangle n - 2 moved to a centroid of +FAR on every axis and triangle n - 1 to -FAR, each keeping its shape;
    shared and never written"""
    if n not in _scenes:
        t = T.soup(n, 11)
        for i, to in ((n - 2, FAR), (n - 1, -FAR)):
            p = t["p"][i].astype(np.float64)
            t["p"][i] = (p - p.mean(axis=0) + to).astype(np.float32)
        t.setflags(write=False)
        _scenes[n] = t
    return _scenes[n]


def host_tree(n, method, tris=None):
    """(WideBVH of far_ends(n) by "linear", "ploc" or "split" — BuildPLOC(radius 8, SPLIT_BUDGET) —, its Woop data); shared and never written.
    tris: other triangles than far_ends(n), not kept"""
    if tris is None and (n, method) in _trees:
        return _trees[n, method]
    t = far_ends(n) if tris is None else tris
    b, s, cfg = api.WideBVH(), api.Scene.FromArrays(t, T.soup_material()), api.InstanceConfig().bvh_params()
    if method == "linear":
        b.BuildLinear(s, cfg)
    else:
        b.BuildPLOC(s, cfg, 8, SPLIT_BUDGET if method == "split" else 0.0)
    b.nodes.setflags(write=False)
    out = (b, api.woop_matrices(t, b.tri_indices))
    if tris is None:
        _trees[n, method] = out
    return out


def centroid_box(tris):
    """(lo [3], hi [3]) of the vertex means"""
    c = tris["p"].astype(np.float64).mean(axis=1)
    return c.min(axis=0), c.max(axis=0)


def rocprim_merge_sort_limit():
    """(merge_sort_limit of the installed rocPRIM's radix_sort_config<>, the header it was read from); (None, why) when no header is found or read"""
    roots = [os.environ.get(k) for k in ("ROCM_PATH", "HIP_PATH", "ROCM_HOME")] + ["/opt/rocm"]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    tried = []
    for root in roots:
        if not root:
            continue
        path = os.path.join(root, "include", "rocprim", "device", "device_radix_sort_config.hpp")
        if path in tried:
            continue
        tried.append(path)
        if not os.path.exists(path):
            continue
        m = re.search(r"MergeSortLimit\s*=\s*([0-9][0-9uUlL\s*']*)[>,]", open(path).read())
        if not m:
            return None, "no default for MergeSortLimit in " + path
        limit = 1
        for factor in m.group(1).split("*"):
            limit *= int(re.sub(r"[uUlL'\s]", "", factor))
        return limit, path
    return None, "no rocPRIM header among " + ", ".join(tried)
