"""-m gpu: adypt_hip --materials-from other.obj (csrc/cli/main.cpp) gives the context the other OBJ's material table and textures
(adypt_multi_set_materials) before the main render: the EXR is, byte for byte, the one of a run whose config names the other OBJ; with --history-from
the swap comes after the history poses.  What the command line refuses without a GPU is in tests/test_cli_options_appearance.py."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402

EXE = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")


def run(*args):
    r = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return r.returncode, r.stdout.decode()


class Other:
    """tiny0 at 64 x 36 and, beside it, the same triangles under another material file: the lamp dark and `green` switched on instead, `white` a glossy illum 2 / Ns 200,
    `red` with a 5 x 3 texture; and a config that names that OBJ"""

    def __init__(self, cache):
        self.spec = scenes.make_scene("tiny0", cache, width=64, height=36)
        d = os.path.dirname(self.spec.obj_path)
        obj = open(self.spec.obj_path).read()
        mtllib = [line.split()[1] for line in obj.splitlines() if line.startswith("mtllib")][0]
        blocks = open(os.path.join(d, mtllib)).read().split("newmtl ")
        rgba = np.full((3, 5, 4), 255, np.uint8)
        rgba[..., :3] = np.random.RandomState(6).randint(0, 256, size=(3, 5, 3))
        api.save_png(os.path.join(d, "tiny0_other_for_cli.png"), rgba)

        def changed(block):
            name = block.split("\n", 1)[0].strip()
            if name == "lamp":
                block = re.sub(r"^Ke .*$", "Ke 0 0 0", block, flags=re.M)
            if name == "green":  # (switched on: with the lamp dark nothing else lights the scene)
                block = re.sub(r"^Ke .*$", "Ke 6 5 4", block, flags=re.M)
            if name == "white":
                block = re.sub(r"^illum .*$", "illum 2", re.sub(r"^Ns .*$", "Ns 200", re.sub(r"^Ks .*$", "Ks 0.5 0.5 0.5", block, flags=re.M), flags=re.M), flags=re.M)
            if name == "red":
                block = block.rstrip("\n") + "\nmap_Kd tiny0_other_for_cli.png\n\n"
            return block
        with open(os.path.join(d, "tiny0_other_for_cli.mtl"), "w") as f:
            f.write("newmtl ".join(changed(b) for b in blocks))
        self.obj = os.path.join(d, "tiny0_other_for_cli.obj")
        with open(self.obj, "w") as f:
            f.write(obj.replace("mtllib " + mtllib, "mtllib tiny0_other_for_cli.mtl"))
        self.config = os.path.join(d, "tiny0_other_for_cli.config")
        with open(self.config, "w") as f:
            f.write(open(self.spec.config_path).read().replace(self.spec.obj_path, self.obj).replace(self.spec.config["bvh_file"], os.path.join(d, "tiny0_other_for_cli.bvh")))
        a, b = api.Scene(), api.Scene()
        assert a.LoadFromFile(self.spec.obj_path) and b.LoadFromFile(self.obj)
        assert a.triangles.tobytes() == b.triangles.tobytes() and a.materials.tobytes() != b.materials.tobytes() and len(b.textures) == 1 and b.textures[0].shape == (3, 5, 3)
        self.n_tris, self.n_mats = a.n_tris, len(b.materials) // 64


_other = []


def other_of(cache):
    if not _other:
        _other.append(Other(cache))
    return _other[0]


def test_cli_materials_from(scene_cache, tmp_path):
    o = other_of(scene_cache)
    tail = ("--spp", "3", "--seed", "5")
    old, swapped, fresh = (str(tmp_path / name) for name in ("old.exr", "swapped.exr", "fresh.exr"))
    code, log = run(o.spec.config_path, *tail, "--out", old)
    assert code == 0 and "[PT]MATERIALS:" not in log, log
    code, log = run(o.spec.config_path, "--materials-from", o.obj, *tail, "--out", swapped)
    assert code == 0, log
    lines = re.findall(r"^\[PT\]MATERIALS: materials (\d+) textures (\d+) reclassed (\d+) of (\d+) triangles$", log, re.M)
    assert len(lines) == 1, log
    m, t, k, n = (int(x) for x in lines[0])
    assert (m, t, n) == (o.n_mats, 1, o.n_tris) and 0 < k < n, log
    code, log = run(o.config, *tail, "--out", fresh)
    assert code == 0, log
    want = open(fresh, "rb").read()
    assert open(swapped, "rb").read() == want, "the run whose config names the other OBJ"
    assert open(old, "rb").read() != want  # the change shows


def test_cli_materials_from_after_the_history_poses(scene_cache, tmp_path):
    o = other_of(scene_cache)
    out, den, kept = (str(tmp_path / name) for name in ("o.exr", "d.exr", "kept.exr"))
    code, log = run(o.spec.config_path, "--materials-from", o.obj, "--spp", "4", "--seed", "5", "--out", out, "--denoise", den, "--history-from", o.spec.config_path, "--rectify",
                    "--rectify-out", kept)
    assert code == 0, log
    assert 0 < log.index("history pose") < log.index("[PT]MATERIALS:") < log.index("[PT]TEMPORAL:"), log
    found = re.search(r"\[PT\]TEMPORAL: history on (\d+) of (\d+) hit pixels", log)
    assert found and int(found.group(1)) > 0, log  # the history of the old light is there for --rectify to judge
    assert os.path.getsize(den) > 0 and os.path.getsize(kept) > 0
