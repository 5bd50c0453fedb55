"""adypt_hip --materials-from where the command line ends before a device is asked for (csrc/cli/options.cpp): the option's place in the synopsis, and
the refusals that exit 2 — a file that cannot be opened, the option given twice, a missing value.  No GPU."""
import os
import subprocess

from adypt_amd import _native as N
from adypt_amd import scenes

EXE = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")


def test_materials_from_option_record(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    out = str(tmp_path / "o.exr")
    missing, missing_config = str(tmp_path / "missing.obj"), str(tmp_path / "missing.config")

    def cli(*args, config=spec.config_path):
        r = subprocess.run([EXE, config] + list(args) + ["--spp", "2", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path))
        return r.returncode, r.stdout.decode()
    code, text = cli("--materials-from", missing)
    assert code == 2 and text == "--materials-from %s: the file cannot be opened\n" % missing, text
    code, text = cli("--materials-from", spec.obj_path, "--materials-from", spec.obj_path)
    assert code == 2 and "--materials-from is given twice" in text, text
    code, text = cli("--materials-from", missing, "--materials-from", spec.obj_path)
    assert code == 2 and "--materials-from is given twice" in text, text
    code, text = cli("--materials-from", "")
    assert code == 2 and "takes the name of an OBJ file" in text, text
    r = subprocess.run([EXE, spec.config_path, "--materials-from"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path))  # (the value is missing)
    assert r.returncode == 2 and b"unknown option --materials-from" in r.stdout
    # what does not go together is said first: the file is looked for last
    code, text = cli("--materials-from", missing, "--rectify")
    assert code == 2 and "--rectify needs a temporal --denoise call" in text, text
    # a file that opens lets the command line through: the tool goes on and fails on the config it is given, before any device
    code, text = cli("--materials-from", spec.obj_path, config=missing_config)
    assert code == 1 and "Invalid instance" in text and "--materials-from" not in text, text
    code, text = cli("--materials-from", spec.obj_path, "--denoise", str(tmp_path / "d.exr"), "--history-from", missing_config, "--rectify")
    assert code == 1 and "Invalid instance" in text, text
    assert not os.listdir(str(tmp_path)), "a refused command line wrote a file"
    usage = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    assert "[--materials-from other.obj]" in usage
