"""-m gpu: adypt_hip --morph-target a.obj --morph-target b.obj --morph-weights w0,w1 (csrc/cli/main.cpp) renders the config's scene with both targets,
diffed against the scene as loaded, blended in on the GPU — alone and under --part-matrices: the image BindParts + BindMorph + Pose(morph_weights=...)
give in this process, bit for bit.  What the command line refuses: tests/test_cli_options.py."""
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
WEIGHTS = (0.5, -0.25)


def run(*args):
    r = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return r.returncode, r.stdout.decode()


def target_obj(spec, name, move):
    """the scene's OBJ with move(x, y, z) in place of every vertex, beside the original so that its mtllib and textures are found"""
    path = os.path.join(os.path.dirname(spec.obj_path), name)
    with open(spec.obj_path) as f, open(path, "w") as g:
        for line in f:
            w = line.split()
            if w and w[0] == "v":
                line = "v %r %r %r\n" % move(*(float(v) for v in w[1:4]))
            g.write(line)
    return path


def test_cli_morph_targets(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    # two targets that move a part of the scene each: the upper half leans, the left side swells
    a_obj = target_obj(spec, "tiny0_morph_a_for_cli.obj", lambda x, y, z: (x + 0.5 * (y - 1.0), y, z) if y > 1.0 else (x, y, z))
    b_obj = target_obj(spec, "tiny0_morph_b_for_cli.obj", lambda x, y, z: (x, y * 1.25, z + 0.5) if x < -1.0 else (x, y, z))
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=5)
    pt = inst.m_path_tracer
    tris = np.array(inst.scene.triangles).view(O.TRI_DT)
    n = len(tris)
    entries = []
    for k, path in enumerate((a_obj, b_obj)):
        target = api.Scene()
        assert target.LoadFromFile(path)
        tri, d = api.morph_diff(tris, target.triangles)
        assert 0 < len(tri) < n
        entries.append((tri, np.full(len(tri), k, np.int32), d))
    tri, tgt, d = (np.concatenate(a) for a in zip(*entries))
    touched = len(np.unique(tri))
    n_mats = len(np.ascontiguousarray(inst.scene.materials).view(O.MAT_DT).reshape(-1))
    loose = (tris["matid"] < 0) | (tris["matid"] >= n_mats)
    parts = np.where(loose, n_mats, tris["matid"]).astype(np.int32)
    n_parts = n_mats + (1 if loose.any() else 0)
    mats = np.stack([P.identity()] * n_parts)
    table = str(tmp_path / "parts.txt")
    with open(table, "w") as f:
        f.write("0 %s\n" % " ".join(repr(float(v)) for v in P.matrix_set(1)[0].reshape(-1)))
    images = []
    for with_table in (False, True):
        if with_table:
            mats[0] = P.matrix_set(1)[0]
        pt.BindParts(parts, n_parts)
        pt.BindMorph(tri, tgt, d, 2)
        pt.Pose(mats, morph_weights=WEIGHTS)
        pt.Trace(True, 3)
        want = pt.ReadResult()
        pt.Pose(mats)
        pt.Trace(True, 3)
        assert not np.array_equal(bits(want), bits(pt.ReadResult()))  # the layer shows
        pt.UnbindPose()
        pt.UpdateTriangles(0, tris["p"].reshape(-1, 9), tris["n"].reshape(-1, 9))  # the scene as loaded again
        out = str(tmp_path / ("morph%d.exr" % with_table))
        code, log = run(spec.config_path, "--morph-target", a_obj, "--morph-target", b_obj, "--morph-weights", ",".join(repr(w) for w in WEIGHTS),
                        *(["--part-matrices", table] if with_table else []), "--spp", "3", "--seed", "5", "--out", out)
        assert code == 0, log
        lines = [line for line in log.splitlines() if line.startswith("[PT]MORPH:")]
        assert lines == ["[PT]MORPH: targets 2 entries %d triangles %d of %d" % (len(tri), touched, n)], log
        assert len(re.findall(r"^\[PT\]POSE:", log, flags=re.M)) == int(with_table)
        assert np.array_equal(bits(api.load_exr(out)), bits(want)), "with --part-matrices" if with_table else "targets alone"
        images.append(want)
    assert not np.array_equal(bits(images[0]), bits(images[1]))
    pt.destroy()

