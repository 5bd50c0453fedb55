"""adypt_hip --denoise-specular where the command line ends before a device is asked for (csrc/cli/options.cpp).  No GPU."""
import os
import subprocess

from adypt_amd import _native as N
from adypt_amd import scenes

EXE = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")


def test_denoise_specular_refusals(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    out, d_exr = str(tmp_path / "o.exr"), str(tmp_path / "d.exr")

    def cli(*args):
        r = subprocess.run([EXE, spec.config_path] + list(args) + ["--spp", "4", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path))
        return r.returncode, r.stdout.decode()
    code, text = cli("--denoise-specular", "4")
    assert code == 2 and "--denoise-specular needs --denoise" in text, text
    for bad in ("0", "9", "-1", "2.0", "x", ""):
        code, text = cli("--denoise", d_exr, "--denoise-specular", bad)
        assert code == 2 and "--denoise-specular takes a number of bounces from 1 to 8" in text, (bad, text)
    code, text = cli("--denoise", d_exr, "--denoise-specular")  # (the value is missing: `--spp` is taken for it)
    assert code == 2, text
    for temporal in (("--history-from", spec.config_path), ("--history-cap", "16"), ("--history-out", str(tmp_path / "h.exr")), ("--history-cap", "16", "--follow-motion"),
                     ("--history-cap", "16", "--rectify")):
        code, text = cli("--denoise", d_exr, "--denoise-specular", "4", *temporal)
        assert code == 2 and "no temporal form" in text, (temporal, text)
    for word in ("--follow-motion", "--rectify"):  # (without a temporal option these are refused for what they lack, as before)
        code, text = cli("--denoise", d_exr, "--denoise-specular", "4", word)
        assert code == 2, (word, text)
    assert not os.listdir(str(tmp_path)), "a refused command line wrote a file"
    code, usage = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode, subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    assert code == 2 and "[--denoise-specular K]" in usage
