"""integration/HipPathTracer.hpp: DenoiseTemporalSpecular, with its defaulted arguments and with every one given, compiles against the reference's own
headers, with the recipe of tests/test_integration_header.py.  Build container only: skipped where /root/reference does not exist (GPU box)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference sources not present")
def test_followed_temporal_call_compiles(tmp_path):
    tracer = tmp_path / "Tracer"
    tracer.mkdir()
    os.symlink(os.path.join(ROOT, "integration", "HipPathTracer.hpp"), tracer / "HipPathTracer.hpp")
    for name in ("Util", "BVH", "InstanceConfig.hpp"):
        os.symlink(os.path.join(REF, "src", name), tmp_path / name)
    (tmp_path / "check.cpp").write_text(
        '#include "Tracer/HipPathTracer.hpp"\n'
        "int use(HipPathTracer &pt)\n"
        "{\n"
        "    std::vector<float> rgb, virtual_position;\n"
        "    const adypt_denoise_params params = {3, 2.0f, 0.2f};\n"
        "    if(!pt.SetNoiseStats(true)) return 1;\n"
        "    pt.Trace(true);\n"
        "    if(!pt.DenoiseTemporalSpecular(&rgb)) return 2;\n"
        "    if(!pt.DenoiseTemporalSpecular(&rgb, 8, 16.0f)) return 3;\n"
        "    pt.Trace(true);\n"
        "    if(!pt.DenoiseTemporalSpecular(&rgb, 8, 16.0f, false, &virtual_position, &params)) return 4;\n"
        "    return (int)(rgb.size() + virtual_position.size());\n"
        "}\n")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-DGLM_FORCE_SWIZZLE", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(REF, "dep"), "-I" + str(tmp_path), str(tmp_path / "check.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
