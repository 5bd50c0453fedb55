"""adypt_hip --rebuild-above: the argument errors, found before any device is asked for.  No GPU."""
import os
import subprocess

from adypt_amd import _native as N
from adypt_amd import scenes


def test_rebuild_above_argument_errors_exit_2(tmp_path):
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    scene = scenes.make_scene("tiny0", str(tmp_path), width=64, height=36)
    out = str(tmp_path / "o.exr")

    def run(*args):
        r = subprocess.run([exe, scene.config_path, "--spp", "1", "--out", out] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        return r.returncode, r.stdout.decode()

    code, log = run("--rebuild-above", "1.4")
    assert code == 2 and "--pose" in log, log
    code, log = run("--pose", scene.obj_path, "--rebuild-above", "1.4", "--rebuild")
    assert code == 2 and "--rebuild" in log, log
    code, log = run("--pose", scene.obj_path, "--rebuild", "--rebuild-method", "ploc", "--rebuild-above", "1.4")
    assert code == 2, log
    for bad in ("nan", "-1", "inf", "much", "1.4x"):
        code, log = run("--pose", scene.obj_path, "--rebuild-above", bad)
        assert code == 2 and "finite number" in log, (bad, log)
    code, log = run("--pose", scene.obj_path, "--rebuild-above", "1.4", "--split-budget", "0.3")
    assert code == 2 and "--split-budget" in log, log
    code, log = run("--pose", scene.obj_path, "--rebuild-above")
    assert code == 2, log
    assert not os.path.exists(out)
