"""-m gpu: adypt_hip --pose moved.obj --rebuild renders the pose on a tree rebuilt on the GPU: the image UpdateTriangles + RebuildBVH give in this
process, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests.helpers import bits  # noqa: E402


def test_cli_pose_and_rebuild(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    moved_obj = os.path.join(os.path.dirname(spec.obj_path), "tiny0_pose_for_rebuild_cli.obj")
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
    t = np.array(moved.triangles).view(O.TRI_DT)
    pt.UpdateTriangles(0, t["p"].reshape(-1, 9), t["n"].reshape(-1, 9))
    info = pt.RebuildBVH(inst.m_config.bvh_params())
    pt.Trace(True, 3)
    want = pt.ReadResult()
    pt.destroy()
    out = str(tmp_path / "rebuilt.exr")
    r = subprocess.run([exe, spec.config_path, "--pose", moved_obj, "--rebuild", "--spp", "3", "--seed", "5", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = r.stdout.decode()
    assert r.returncode == 0, log
    assert "554 triangles moved, refit" in log and "rebuild: %d nodes, 554 references, %d levels" % (info["n_nodes"], info["levels"]) in log, log
    assert log.index("triangles moved, refit") < log.index("rebuild:")  # the pose first
    assert np.array_equal(bits(api.load_exr(out)), bits(want))
