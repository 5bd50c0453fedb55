"""integration/HipPathTracer.hpp: BindParts, BindSkin, Pose (its PosePolicy overload too) and UnbindPose compile against the reference's own headers, with
the recipe of tests/test_integration_header.py.  Build container only: skipped where /root/reference does not exist (GPU box)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference sources not present")
def test_bind_and_pose_compile(tmp_path):
    tracer = tmp_path / "Tracer"
    tracer.mkdir()
    os.symlink(os.path.join(ROOT, "integration", "HipPathTracer.hpp"), tracer / "HipPathTracer.hpp")
    for name in ("Util", "BVH", "InstanceConfig.hpp"):
        os.symlink(os.path.join(REF, "src", name), tmp_path / name)
    (tmp_path / "check.cpp").write_text(
        '#include "Tracer/HipPathTracer.hpp"\n'
        "int use(HipPathTracer &pt, const Scene &scene, const adypt_bvh_params *bvh_cfg)\n"
        "{\n"
        "    const size_t n = scene.GetTriangles().size();\n"
        "    std::vector<int32_t> parts(n, 0);\n"
        "    std::vector<uint16_t> joints(n * 12, 0);\n"
        "    std::vector<float> weights(n * 12, 0.25f), matrices(2 * 12, 0.0f);\n"
        "    adypt_pose_outcome outcome;\n"
        "    if(!pt.BindParts(parts, 2)) return 1;\n"
        "    if(!pt.Pose(matrices)) return 2;\n"
        "    if(!pt.BindSkin(joints, weights, 2)) return 3;\n"
        "    if(!pt.Pose(matrices, HipPathTracer::PosePolicy(1.5))) return 4;\n"
        "    if(!pt.Pose(matrices, HipPathTracer::PosePolicy(0.0, HipPathTracer::RebuildMethod::Linear), &outcome, bvh_cfg)) return 5;\n"
        "    if(!pt.UnbindPose()) return 6;\n"
        "    pt.Trace(true);\n"
        "    return pt.GetSPP() + outcome.rebuilt;\n"
        "}\n")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-DGLM_FORCE_SWIZZLE", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(REF, "dep"), "-I" + str(tmp_path), str(tmp_path / "check.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
