"""adypt_hip --follow-specular where the command line ends before a device is asked for (csrc/cli/options.cpp).  No GPU."""
import os
import subprocess

from adypt_amd import _native as N
from adypt_amd import scenes

EXE = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")


def test_follow_specular_refusals(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    out, d_exr = str(tmp_path / "o.exr"), str(tmp_path / "d.exr")

    def cli(*args):
        r = subprocess.run([EXE, spec.config_path] + list(args) + ["--spp", "4", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path))
        return r.returncode, r.stdout.decode()
    # it needs a temporal --denoise call
    for args in (("--follow-specular", "4"), ("--denoise", d_exr, "--follow-specular", "4"), ("--history-cap", "16", "--follow-specular", "4")):
        code, text = cli(*args)
        assert code == 2, (args, text)
    code, text = cli("--denoise", d_exr, "--follow-specular", "4")
    assert "--follow-specular needs a temporal --denoise call" in text, text
    for bad in ("0", "9", "-1", "2.0", "x", ""):
        code, text = cli("--denoise", d_exr, "--history-cap", "16", "--follow-specular", bad)
        assert code == 2 and "--follow-specular takes a number of bounces from 1 to 8" in text, (bad, text)
    code, text = cli("--denoise", d_exr, "--history-cap", "16", "--follow-specular")  # (the value is missing: `--spp` is taken for it)
    assert code == 2, text
    # what it does not combine with
    for word in (("--follow-motion",), ("--rectify",), ("--denoise-moments",)):
        code, text = cli("--denoise", d_exr, "--history-cap", "16", "--follow-specular", "4", *word)
        assert code == 2 and "--follow-specular does not combine with" in text, (word, text)
    code, text = cli("--denoise", d_exr, "--history-cap", "16", "--follow-specular", "4", "--denoise-specular", "4")
    assert code == 2 and "no temporal form" in text, text  # (--denoise-specular's own refusal comes first, as before)
    assert not os.listdir(str(tmp_path)), "a refused command line wrote a file"
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 2 and "[--follow-specular K]" in r.stdout.decode()
