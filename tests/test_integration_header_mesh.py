"""integration/HipPathTracer.hpp: BindMesh, PoseVertices (with and without normals, with and without PosePolicy) and UnbindMesh compile against the
reference's own headers as C++11, with the recipe of tests/test_integration_header_pose.py.  Build container only: skipped where /root/reference
does not exist (GPU box)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference sources not present")
def test_bind_mesh_and_pose_vertices_compile(tmp_path):
    tracer = tmp_path / "Tracer"
    tracer.mkdir()
    os.symlink(os.path.join(ROOT, "integration", "HipPathTracer.hpp"), tracer / "HipPathTracer.hpp")
    for name in ("Util", "BVH", "InstanceConfig.hpp"):
        os.symlink(os.path.join(REF, "src", name), tmp_path / name)
    (tmp_path / "check.cpp").write_text(
        '#include "Tracer/HipPathTracer.hpp"\n'
        "#include <adypt_host.h>\n"
        "int use(HipPathTracer &pt, const Scene &scene, const adypt_bvh_params *bvh_cfg)\n"
        "{\n"
        "    const size_t n = scene.GetTriangles().size();\n"
        "    std::vector<int32_t> indices(3 * n);\n"
        "    const int64_t n_vertices = adypt_weld_triangles(scene.GetTriangles().data(), (int64_t)n, indices.data(), nullptr, nullptr);\n"
        "    std::vector<float> positions(3 * (size_t)n_vertices, 0.0f), normals(3 * (size_t)n_vertices, 1.0f);\n"
        "    adypt_weld_triangles(scene.GetTriangles().data(), (int64_t)n, nullptr, positions.data(), normals.data());\n"
        "    adypt_pose_outcome outcome;\n"
        "    if(!pt.BindMesh(indices, n_vertices)) return 1;\n"
        "    if(!pt.PoseVertices(positions)) return 2;\n"
        "    if(!pt.PoseVertices(positions, normals)) return 3;\n"
        "    if(!pt.PoseVertices(positions, normals, HipPathTracer::PosePolicy(1.5))) return 4;\n"
        "    if(!pt.PoseVertices(positions, std::vector<float>(), HipPathTracer::PosePolicy(0.0, HipPathTracer::RebuildMethod::Linear), &outcome, bvh_cfg)) return 5;\n"
        "    if(!pt.UnbindMesh()) return 6;\n"
        "    pt.Trace(true);\n"
        "    return pt.GetSPP() + outcome.rebuilt;\n"
        "}\n")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-DGLM_FORCE_SWIZZLE", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(REF, "dep"), "-I" + str(tmp_path), str(tmp_path / "check.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
