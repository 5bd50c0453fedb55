"""integration/HipPathTracer.hpp: SetTriangles and the Initialize overload without a WideBVH compile against the reference's own headers, with the recipe
of tests/test_integration_header.py.  Build container only: skipped where /root/reference does not exist (GPU box)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference sources not present")
def test_set_triangles_and_initialize_without_a_bvh_compile(tmp_path):
    tracer = tmp_path / "Tracer"
    tracer.mkdir()
    os.symlink(os.path.join(ROOT, "integration", "HipPathTracer.hpp"), tracer / "HipPathTracer.hpp")
    for name in ("Util", "BVH", "InstanceConfig.hpp"):
        os.symlink(os.path.join(REF, "src", name), tmp_path / name)
    (tmp_path / "check.cpp").write_text(
        '#include "Tracer/HipPathTracer.hpp"\n'
        "int use(const InstanceConfig::PT *cfg, const Scene &scene, const adypt_bvh_params *bvh_cfg)\n"
        "{\n"
        "    HipPathTracer pt;\n"
        "    adypt_rebuild_info info;\n"
        "    if(!pt.Initialize(cfg, scene, 1920, 1080)) return 1;\n"
        "    if(!pt.Initialize(cfg, scene, 1920, 1080, std::vector<int>(2, 0), 0, bvh_cfg, HipPathTracer::RebuildMethod::Linear, 8, 0.0, &info)) return 2;\n"
        "    std::vector<Triangle> fewer(scene.GetTriangles().begin(), scene.GetTriangles().begin() + 1);\n"
        "    if(!pt.SetTriangles(fewer)) return 3;\n"
        "    if(!pt.SetTriangles(scene.GetTriangles(), bvh_cfg, &info, HipPathTracer::RebuildMethod::PLOC, 16, 0.3)) return 4;\n"
        "    pt.Trace(true);\n"
        "    return pt.GetSPP() + (int)info.n_nodes;\n"
        "}\n")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-DGLM_FORCE_SWIZZLE", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(REF, "dep"), "-I" + str(tmp_path), str(tmp_path / "check.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
