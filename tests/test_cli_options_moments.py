"""adypt_hip --denoise-moments where the command line ends before a device is asked for (csrc/cli/options.cpp): the flag, the floor of --spp, the
three combinations that exit 2.  No GPU."""
import os
import subprocess

from adypt_amd import _native as N
from adypt_amd import scenes

EXE = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")


def test_denoise_moments_option_record(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    out, d_exr, v_exr = str(tmp_path / "o.exr"), str(tmp_path / "d.exr"), str(tmp_path / "v.exr")
    missing = str(tmp_path / "missing.config")

    def cli(*args, spp="1"):
        r = subprocess.run([EXE, spec.config_path] + list(args) + ["--spp", spp, "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path))
        return r.returncode, r.stdout.decode()
    temporal = ("--denoise", d_exr, "--history-cap", "16")
    # the three combinations: no temporal --denoise call, --rectify, --denoise-specular
    for args in (("--denoise-moments",), ("--denoise", d_exr, "--denoise-moments")):
        code, text = cli(*args)
        assert code == 2 and "--denoise-moments needs a temporal --denoise call" in text, (args, text)
    code, text = cli(*temporal, "--denoise-moments", "--rectify")
    assert code == 2 and "--denoise-moments does not combine with --rectify" in text, text
    code, text = cli("--denoise", d_exr, "--denoise-moments", "--denoise-specular", "4")
    assert code == 2 and "--denoise-moments does not combine with --denoise-specular" in text, text
    code, text = cli(*temporal, "--denoise-moments", "--denoise-specular", "4")
    assert code == 2 and "--denoise-moments does not combine with --denoise-specular" in text, text
    code, text = cli(*temporal, "--variance-out", v_exr)
    assert code == 2 and "--variance-out needs --denoise-moments" in text, text
    code, text = cli(*temporal, "--denoise-moments", "--variance-out")  # (the value is missing: `--spp` is taken for it, and `1` is no option)
    assert code == 2, text
    # the floor of --spp: 1 with the flag (the command line is accepted: the tool goes on and fails on the config it is given), 0 never; 2 without it
    code, text = cli(*temporal, "--denoise-moments", spp="0")
    assert code == 2 and "needs --spp >= 1" in text, text
    code, text = cli(*temporal, "--denoise-moments", "--primary", "0")
    assert code == 2 and "needs --spp >= 1 and no --primary" in text, text
    for extra in ((), ("--follow-motion",), ("--variance-out", v_exr)):
        code, text = cli(*temporal, "--denoise-moments", "--history-from", missing, *extra)
        assert code == 1 and "Invalid instance" in text and "--spp" not in text, (extra, code, text)
    code, text = cli(*temporal)
    assert code == 2 and text == "--denoise needs --spp >= 2 and no --primary\n", text
    code, text = cli(*temporal, "--history-from", missing, spp="2")
    assert code == 1 and "Invalid instance" in text, text
    assert not os.listdir(str(tmp_path)), "a refused command line wrote a file"
    usage = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    assert "[--denoise-moments [--variance-out v.exr]]" in usage
