"""-m gpu: adypt_hip --part-matrices FILE (csrc/cli/main.cpp) renders the config's scene with every material's triangles moved by that part's matrix on
the GPU: the image BindParts + Pose give in this process, bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import pose_truth as P  # noqa: E402
from tests.helpers import bits  # noqa: E402

EXE = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")


def test_cli_part_matrices(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=5)
    pt = inst.m_path_tracer
    pt.Trace(True, 3)
    rest_image = pt.ReadResult()
    matid = np.array(inst.scene.triangles).view(O.TRI_DT)["matid"]
    n_mats = len(np.ascontiguousarray(inst.scene.materials).view(O.MAT_DT).reshape(-1))
    loose = (matid < 0) | (matid >= n_mats)
    parts = np.where(loose, n_mats, matid).astype(np.int32)
    n_parts = n_mats + (1 if loose.any() else 0)
    assert n_parts >= 2
    # every other part moves; the rest is not listed and stays
    mats = np.stack([P.identity()] * n_parts)
    moving = P.matrix_set(3)
    listed = {}
    for k in range(0, n_parts, 2):
        mats[k] = listed[k] = moving[(k // 2) % 3]
    pt.BindParts(parts, n_parts)
    pt.Pose(mats)
    pt.Trace(True, 3)
    want = pt.ReadResult()
    assert not np.array_equal(bits(want), bits(rest_image))
    pt.destroy()
    table = str(tmp_path / "parts.txt")
    with open(table, "w") as f:
        f.write("# part m00 m01 m02 m03 m10 ... m23\n\n")
        for k, m in listed.items():
            f.write("%d %s\n" % (k, " ".join(repr(float(v)) for v in m.reshape(-1))))
    out = str(tmp_path / "pose.exr")
    r = subprocess.run([EXE, spec.config_path, "--part-matrices", table, "--spp", "3", "--seed", "5", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = r.stdout.decode()
    assert r.returncode == 0, log
    lines = [line for line in log.splitlines() if line.startswith("[PT]POSE:")]
    assert len(lines) == 1 and re.match(r"\[PT\]POSE: parts %d triangles %d " % (n_parts, len(matid)), lines[0]), log
    assert np.array_equal(bits(api.load_exr(out)), bits(want))
    # (two ways to move the scene at once, a part the scene does not have: tests/test_cli_options.py)
