"""-m gpu: adypt_hip --build gpu (csrc/cli/main.cpp): no .bvh cache, no host build; the first tree is built on the GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from tests.helpers import bits  # noqa: E402

EXE = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")


def bvh_files(root):
    return [f for d, _, fs in os.walk(root) for f in fs if f.endswith(".bvh")]


def test_cli_build_gpu(tmp_path):
    """adypt_hip --build gpu renders on the tree Instance.Initialize(build_on_gpu=True) builds in this process, says so, and leaves no .bvh behind"""
    spec = scenes.make_scene("tiny0", str(tmp_path / "scene"), width=32, height=18)
    assert not bvh_files(str(tmp_path))
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=5, build_on_gpu=True)
    pt = inst.m_path_tracer
    info = pt.build_info
    pt.Trace(True, 4)
    want = pt.ReadResult()
    # the same image as on the host's PLOC tree, uploaded
    b = api.WideBVH()
    b.BuildPLOC(inst.scene, inst.m_config.bvh_params())
    assert (info["n_nodes"], info["n_refs"]) == (len(b.nodes) // 80, len(b.tri_indices))
    pt.destroy()
    inst.m_hipscene.Initialize(inst.scene, b)
    pt.Initialize(inst.m_config.pt_params(5), inst.m_hipscene, 32, 18)
    ip, iv = inst.m_camera.matrices()
    pt.SetCamera(ip, iv, inst.m_camera.position)
    pt.Trace(True, 4)
    assert pt.build_info is None and np.array_equal(bits(pt.ReadResult()), bits(want))
    pt.destroy()
    out = str(tmp_path / "a.exr")
    r = subprocess.run([EXE, spec.config_path, "--build", "gpu", "--spp", "4", "--seed", "5", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = r.stdout.decode()
    assert r.returncode == 0, log
    lines = [line for line in log.splitlines() if line.startswith("[PT]BUILD:")]
    assert len(lines) == 1, log
    assert re.match(r"\[PT\]BUILD: %d nodes, %d references, %d levels, method ploc radius 8, [0-9.]+ ms" % (info["n_nodes"], info["n_refs"], info["levels"]), lines[0]), lines[0]
    assert "[SBVH]" not in log and "rebuild:" not in log
    assert np.array_equal(bits(api.load_exr(out)), bits(want))
    assert not bvh_files(str(tmp_path)), "no .bvh file is left behind"
    # the method and the pose policy after it
    r = subprocess.run([EXE, spec.config_path, "--build", "gpu", "--rebuild-method", "linear", "--spp", "1", "--seed", "5", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and "method linear" in r.stdout.decode() and not bvh_files(str(tmp_path)), r.stdout.decode()
    r = subprocess.run([EXE, spec.config_path, "--build", "gpu", "--ploc-radius", "40", "--spp", "1", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 1 and "radius" in r.stdout.decode()
