"""integration/HipPathTracer.hpp: PlanByHistory and TraceByHistory, with their defaulted arguments and with every one given, compile against the
reference's own headers, with the recipe of tests/test_integration_header.py.  Build container only: skipped where /root/reference does not exist
(GPU box)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference sources not present")
def test_plan_and_trace_by_history_compile(tmp_path):
    tracer = tmp_path / "Tracer"
    tracer.mkdir()
    os.symlink(os.path.join(ROOT, "integration", "HipPathTracer.hpp"), tracer / "HipPathTracer.hpp")
    for name in ("Util", "BVH", "InstanceConfig.hpp"):
        os.symlink(os.path.join(REF, "src", name), tmp_path / name)
    (tmp_path / "check.cpp").write_text(
        '#include "Tracer/HipPathTracer.hpp"\n'
        "int use(HipPathTracer &pt)\n"
        "{\n"
        "    std::vector<float> rgb, reach;\n"
        "    adypt_history_plan plan;\n"
        "    if(!pt.SetNoiseStats(true)) return 1;\n"
        "    if(!pt.PlanByHistory(16)) return 2;\n"
        "    if(!pt.PlanByHistory(16, &plan, &reach, 2, 32, 2, 0, 16.0f, true, true)) return 3;\n"
        "    if(!pt.TraceByHistory(16)) return 4;\n"
        "    if(!pt.DenoiseTemporal(&rgb)) return 5;\n"
        "    if(!pt.TraceByHistory(8, &plan, &reach, 2, 16, 4, 31, 64.0f, false, false)) return 6;\n"
        "    return (int)(rgb.size() + reach.size()) + plan.blocks + plan.want_max + (int)plan.pixel_samples;\n"
        "}\n")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-DGLM_FORCE_SWIZZLE", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(REF, "dep"), "-I" + str(tmp_path), str(tmp_path / "check.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
