"""adypt_hip --pose: a pose with another triangle count is an error, found before any device is asked for.  No GPU."""
import os
import subprocess

from adypt_amd import _native as N
from adypt_amd import scenes


def test_pose_with_another_triangle_count_is_refused(tmp_path):
    exe = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
    scene = scenes.make_scene("tiny0", str(tmp_path), width=64, height=36)
    other = scenes.make_scene("tiny2", str(tmp_path), width=64, height=36)
    r = subprocess.run([exe, scene.config_path, "--pose", other.obj_path, "--spp", "1", "--out", str(tmp_path / "o.exr")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = r.stdout.decode()
    assert r.returncode == 1 and "has 5 triangles, the scene has 554" in log, log
    assert not os.path.exists(str(tmp_path / "o.exr"))
    r = subprocess.run([exe, scene.config_path, "--pose", str(tmp_path / "missing.obj")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 1 and b"Unable to load pose" in r.stdout
