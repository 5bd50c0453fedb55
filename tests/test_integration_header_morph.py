"""integration/HipPathTracer.hpp: BindMorph, UnbindMorph and the Pose overloads that take morph weights (with and without PosePolicy) compile against
the reference's own headers as C++11, with the recipe of tests/test_integration_header_pose.py.  Build container only: skipped where /root/reference
does not exist (GPU box)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference sources not present")
def test_bind_morph_and_pose_compile(tmp_path):
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
        "    std::vector<int32_t> parts(n, 0), entry_triangles(4, 0), entry_targets(4, 0);\n"
        "    std::vector<float> deltas(4 * 18, 0.125f), matrices(12, 0.0f), morph_weights(2, 0.5f);\n"
        "    for(int e = 0; e < 4; ++e) { entry_triangles[e] = e / 2; entry_targets[e] = e % 2; }\n"
        "    adypt_pose_outcome outcome;\n"
        "    if(!pt.BindParts(parts, 1)) return 1;\n"
        "    if(!pt.BindMorph(entry_triangles, entry_targets, deltas, 2)) return 2;\n"
        "    if(!pt.Pose(matrices, morph_weights)) return 3;\n"
        "    if(!pt.Pose(matrices)) return 4;\n"
        "    if(!pt.Pose(matrices, morph_weights, HipPathTracer::PosePolicy(1.5))) return 5;\n"
        "    if(!pt.Pose(matrices, morph_weights, HipPathTracer::PosePolicy(0.0, HipPathTracer::RebuildMethod::Linear), &outcome, bvh_cfg)) return 6;\n"
        "    if(!pt.Pose(matrices, HipPathTracer::PosePolicy(1.5))) return 7;\n"
        "    if(!pt.UnbindMorph()) return 8;\n"
        "    if(!pt.UnbindPose()) return 9;\n"
        "    pt.Trace(true);\n"
        "    return pt.GetSPP() + outcome.rebuilt;\n"
        "}\n")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-DGLM_FORCE_SWIZZLE", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(REF, "dep"), "-I" + str(tmp_path), str(tmp_path / "check.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
