"""integration/HipPathTracer.hpp: SetMaterials (with and without textures), UpdateTexture and SetTriangleAttributes compile against the reference's
own headers as C++11, with the recipe of tests/test_integration_header_mesh.py.  Build container only: skipped where /root/reference does not
exist (GPU box)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference sources not present")
def test_appearance_calls_compile(tmp_path):
    tracer = tmp_path / "Tracer"
    tracer.mkdir()
    os.symlink(os.path.join(ROOT, "integration", "HipPathTracer.hpp"), tracer / "HipPathTracer.hpp")
    for name in ("Util", "BVH", "InstanceConfig.hpp"):
        os.symlink(os.path.join(REF, "src", name), tmp_path / name)
    (tmp_path / "check.cpp").write_text(
        '#include "Tracer/HipPathTracer.hpp"\n'
        "int use(HipPathTracer &pt, const Scene &scene)\n"
        "{\n"
        "    const size_t n = scene.GetTriangles().size();\n"
        "    std::vector<HipPathTracer::GPUMaterial> materials(3);\n"
        "    materials[1].m_illum = 2; materials[1].m_shininess = 200.0f; materials[2].m_dtex = 0;\n"
        "    std::vector<uint8_t> pixels(5 * 3 * 3, 128);\n"
        "    std::vector<adypt_texture> textures(1);\n"
        "    textures[0].width = 5; textures[0].height = 3; textures[0].rgb = pixels.data();\n"
        "    adypt_appearance_info info;\n"
        "    if(!pt.SetMaterials(materials)) return 1;\n"
        "    if(!pt.SetMaterials(materials, textures, &info)) return 2;\n"
        "    if(!pt.UpdateTexture(0, pixels.data(), 5, 3)) return 3;\n"
        "    if(!pt.SetTriangleAttributes(0, std::vector<int32_t>(n, 1))) return 4;\n"
        "    if(!pt.SetTriangleAttributes(0, std::vector<int32_t>(), std::vector<float>(6 * n, 0.5f), &info)) return 5;\n"
        "    if(!pt.SetTriangleAttributes(1, std::vector<int32_t>(2, 0), std::vector<float>(12, 0.25f))) return 6;\n"
        "    pt.Trace(true);\n"
        "    return pt.GetSPP() + (int)info.reclassed + info.n_textures;\n"
        "}\n")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-DGLM_FORCE_SWIZZLE", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(REF, "dep"), "-I" + str(tmp_path), str(tmp_path / "check.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
