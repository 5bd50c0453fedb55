"""-m gpu: adypt_hip --pose moved.obj --rebuild-above R keeps the refitted tree for a near pose and rebuilds for a far one, says which, and renders the
image the same calls give in this process, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests.helpers import bits  # noqa: E402


def pose_file(spec, name, move):
    """The scene's OBJ with the vertices of face k at move(k, x, y, z): every face gets vertices of its own, written in front of it, so that faces
    can move apart; normals, texture coordinates, groups and materials stay.  Beside the original, so that its mtllib and textures are found."""
    path = os.path.join(os.path.dirname(spec.obj_path), name)
    lines = open(spec.obj_path).read().split("\n")
    v = [tuple(float(x) for x in line.split()[1:4]) for line in lines if line.startswith("v ")]
    n_v, face = len(v), 0
    with open(path, "w") as g:
        for line in lines:
            w = line.split()
            if w and w[0] == "f":
                assert len(w) == 4, "a face that is no triangle"
                corners = []
                for c in w[1:]:
                    parts = c.split("/")
                    g.write("v %r %r %r\n" % move(face, *v[int(parts[0]) - 1]))
                    n_v += 1
                    corners.append("/".join([str(n_v)] + parts[1:]))
                line = "f " + " ".join(corners)
                face += 1
            g.write(line + "\n")
    return path


@pytest.mark.parametrize("far", [False, True])
def test_cli_rebuild_above(far, tmp_path):
    # a tree without spatial splits, in a directory of its own (the cached .bvh of the shared one has them): refitted in its rest pose it costs what it cost
    spec = scenes.make_scene("tiny0", str(tmp_path), width=64, height=36, bvh={"maxSpatialDepth": 0})
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=5)
    rest = np.array(inst.scene.triangles).view(O.TRI_DT)
    extent = float(rest["p"][..., 0].max()) - float(rest["p"][..., 0].min())
    if far:    # every odd triangle apart by 1.5 extents
        path = pose_file(spec, "tiny0_far_pose_for_cli.obj", lambda face, x, y, z: (x + 1.5 * extent * (face % 2), y, z))
    else:      # a small shear of everything
        path = pose_file(spec, "tiny0_near_pose_for_cli.obj", lambda face, x, y, z: (x + 0.01 * y, y, z))
    moved = api.Scene()
    assert moved.LoadFromFile(path)
    t = np.array(moved.triangles).view(O.TRI_DT)
    assert len(t) == len(rest)
    built = inst.bvh.Cost(inst.m_config.bvh_params())
    pt = inst.m_path_tracer
    pt.UpdateTriangles(0, t["p"].reshape(-1, 9), t["n"].reshape(-1, 9))
    kept_cost = pt.GetTreeCost(inst.m_config.bvh_params())
    ratio = kept_cost["cost"] / built["cost"]
    assert (ratio > 1.4) == far
    if far:
        pt.RebuildBVH(inst.m_config.bvh_params(), "ploc")
    pt.Trace(True, 3)
    want = pt.ReadResult()
    pt.destroy()
    out = str(tmp_path / "o.exr")
    r = subprocess.run([exe, spec.config_path, "--pose", path, "--rebuild-above", "1.4", "--rebuild-method", "ploc", "--spp", "3", "--seed", "5", "--out", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = r.stdout.decode()
    assert r.returncode == 0, log
    line = [x for x in log.split("\n") if "pose policy:" in x]
    assert len(line) == 1 and log.index("triangles moved, refit") < log.index("pose policy:"), log
    assert "tree cost %.4f -> %.4f (ratio %.4f" % (built["cost"], kept_cost["cost"], ratio) in line[0], log
    if far:
        assert ": rebuilt (" in line[0] and "method ploc radius 8" in line[0] and "554 references" in line[0], log
    else:
        assert line[0].endswith(": kept"), log
    assert "[PT]INFO: rebuild:" not in log
    assert np.array_equal(bits(api.load_exr(out)), bits(want))
