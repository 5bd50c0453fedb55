"""-m gpu: adypt_hip --pose moved.obj renders the config's scene, with the tree built for its rest pose, in the pose of moved.obj: the image UpdateTriangles
gives in this process, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests.helpers import bits  # noqa: E402


def test_cli_pose(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    # the same OBJ with every vertex moved: beside the original, so that its mtllib and textures are found
    moved_obj = os.path.join(os.path.dirname(spec.obj_path), "tiny0_pose_for_cli.obj")
    with open(spec.obj_path) as f, open(moved_obj, "w") as g:
        for line in f:
            w = line.split()
            if w and w[0] == "v":
                x, y, z = (float(v) for v in w[1:4])
                line = "v %r %r %r\n" % (x * 1.125, y + 0.25 * x, z - 0.5)
            g.write(line)
    moved = api.Scene()
    assert moved.LoadFromFile(moved_obj)
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=5)
    pt = inst.m_path_tracer
    pt.Trace(True, 3)
    rest_image = pt.ReadResult()
    t = np.array(moved.triangles).view(O.TRI_DT)
    assert len(t) == inst.scene.n_tris
    pt.UpdateTriangles(0, t["p"].reshape(-1, 9), t["n"].reshape(-1, 9))
    pt.Trace(True, 3)
    want = pt.ReadResult()
    assert not np.array_equal(bits(want), bits(rest_image))
    pt.destroy()
    out = str(tmp_path / "pose.exr")
    r = subprocess.run([exe, spec.config_path, "--pose", moved_obj, "--spp", "3", "--seed", "5", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = r.stdout.decode()
    assert r.returncode == 0, log
    assert "554 triangles moved, refit" in log, log
    assert np.array_equal(bits(api.load_exr(out)), bits(want))
