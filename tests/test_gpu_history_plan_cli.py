"""-m gpu: adypt_hip --history-samples with two --history-from poses on tiny0 100x75 against the same sequence through the Python API: the
[PT]PLAN: line, --plan-out, --reach-out, the image and the denoised EXR; the same command line without the flag is what it was."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api  # noqa: E402
from tests import history_reach_truth as HT  # noqa: E402
from tests import test_gpu_denoise_temporal as TG  # noqa: E402
from tests import test_gpu_noise as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "adypt_amd", "adypt_hip")
CASE = G.CASES[0]
SEED, SPP, TARGET = TG.SEED, 8, 20
same = TG.same


def test_cli(scene_cache, tmp_path):
    name, w, h = CASE[:3]
    inst, spec = G._instance(scene_cache, CASE)
    p, cfg, c = inst.m_path_tracer, inst.m_config, inst.m_config.c
    p.SetNoiseStats(True)
    main = json.load(open(spec.config_path))
    # the earlier poses: two and one step away from the main config's camera, with the seeds the tool gives them; through the API as the tool runs them
    paths = []
    for k in (1, 2):
        pos, yaw = TG.camera_of(c, name, 3 - k)
        other = json.loads(json.dumps(main))
        other["camera"]["position"], other["camera"]["yaw"] = pos, yaw
        paths.append(str(tmp_path / ("pose%d.config" % k)))
        json.dump(other, open(paths[-1], "w"), indent=4)
        TG.set_pose(p, cfg, pos, yaw, SEED + k, SPP)
        p.Denoise(temporal=True)
    pos, yaw = TG.camera_of(c, name, 0)
    TG.set_pose(p, cfg, pos, yaw, SEED, 0)
    info = p.TraceByHistory(TARGET, max_spp=SPP)
    image, reach, want = p.ReadResult(), p.ReadHistoryReach(), p.ReadSamplePlan()[1]
    den = p.Denoise(temporal=True)
    assert len(set(want)) >= 2 and info["pixel_samples"] < SPP * w * h, "the case: the plan is not uniform (%s)" % want
    TG.set_pose(p, cfg, pos, yaw, SEED, SPP)
    uniform = p.ReadResult()
    p.destroy()
    out, d_exr, r_exr, p_exr = (str(tmp_path / f) for f in ("o.exr", "d.exr", "reach.exr", "want.exr"))
    copy = str(tmp_path / "main.config")  # (the tool writes its config back on exit)
    json.dump(main, open(copy, "w"), indent=4)

    def cli(*args):
        r = subprocess.run([CLI, copy, "--out", out, "--seed", str(SEED), "--spp", str(SPP), "--denoise", d_exr, "--history-from", paths[0], "--history-from", paths[1]] + list(args),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        return r.returncode, (r.stdout + r.stderr).decode()
    code, text = cli("--history-samples", str(TARGET), "--reach-out", r_exr, "--plan-out", p_exr)
    assert code == 0 and "Saved denoised image (5 levels)" in text, text[-2000:]
    line = "[PT]PLAN: blocks %d want %d..%d pixel_samples %d (uniform %d) with_history %d of %d mean_reach %.3f\n" % (
        info["blocks"], info["want_min"], info["want_max"], info["pixel_samples"], TARGET * w * h, info["pixels_with_history"], w * h, info["mean_reach"])
    assert line in text, (line, text[-2000:])
    assert same(api.load_exr(out), image) and same(api.load_exr(d_exr), den), "the tool's images are not the API's"
    assert same(api.load_exr(r_exr)[..., 0], reach) and same(api.load_exr(p_exr)[..., 0], HT.per_pixel(want, w, h).astype(np.float32))
    # without the flag: the uniform render, and no such line
    code, text = cli()
    assert code == 0 and "[PT]PLAN:" not in text and same(api.load_exr(out), uniform), text[-2000:]
