"""-m gpu: adypt_hip --pose moved.obj --by-vertices [--recompute-normals] (csrc/cli/main.cpp) takes the pose of --pose moved.obj by the mesh binding: the
scene as loaded is welded and bound, and one position (and normal) per vertex crosses the bus.  Both roads write the same EXR, byte for byte; with
--recompute-normals and a moved.obj without normals the device computes the normals the other file carries.  What the command line refuses is here
and, without a GPU, in tests/test_mesh_cli_refusals.py."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import mesh_truth as M  # noqa: E402

EXE = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")


def run(*args):
    r = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return r.returncode, r.stdout.decode()


def write_obj(path, mtllib, idx, positions, normals=None, torn=None):
    """the mesh as an OBJ whose triangles come in the order of idx; torn = (triangle, corner): that corner gets a vertex of its own, somewhere else"""
    num = lambda a: " ".join(repr(float(x)) for x in a)  # noqa: E731  (a binary32 as the shortest decimal that names its binary64: read back exactly)
    with open(path, "w") as f:
        f.write("mtllib %s\n" % mtllib)
        f.write("".join("v %s\n" % num(p) for p in positions))
        if torn is not None:
            f.write("v %s\n" % num(positions[idx[torn]] + np.float32(0.25)))
        if normals is not None:
            f.write("".join("vn %s\n" % num(n) for n in normals))
        for t, tri in enumerate(idx + 1):
            v = [len(positions) + 1 if torn == (t, c) else tri[c] for c in range(3)]
            f.write("f " + " ".join("%d" % v[c] if normals is None else "%d//%d" % (v[c], tri[c]) for c in range(3)) + "\n")


class Pose:
    """tiny0 at 64 x 36, welded, and its pose as OBJ files beside the scene's own (so that its mtllib is found): with the normals api.mesh_normals
    computes, without normals, and torn"""

    def __init__(self, cache):
        self.spec = scenes.make_scene("tiny0", cache, width=64, height=36)
        scene = api.Scene()
        assert scene.LoadFromFile(self.spec.obj_path)
        self.tris = np.array(scene.triangles).view(O.TRI_DT)
        self.idx, rest, _ = api.weld_triangles(self.tris)
        self.positions = M.deform(rest, 3)
        self.normals = api.mesh_normals(self.idx, self.positions)
        mtllib = [line.split()[1] for line in open(self.spec.obj_path) if line.startswith("mtllib")][0]
        d = os.path.dirname(self.spec.obj_path)
        self.with_normals, self.without, self.torn = (os.path.join(d, "tiny0_mesh_%s_for_cli.obj" % k) for k in ("normals", "bare", "torn"))
        write_obj(self.with_normals, mtllib, self.idx, self.positions, self.normals)
        write_obj(self.without, mtllib, self.idx, self.positions)
        write_obj(self.torn, mtllib, self.idx, self.positions, self.normals, torn=(len(self.idx) // 2, 1))
        # the file is the pose, bit for bit
        moved = api.Scene()
        assert moved.LoadFromFile(self.with_normals)
        want = api.mesh_triangles(self.tris, self.idx, self.positions, self.normals).view(O.TRI_DT)
        got = np.array(moved.triangles).view(O.TRI_DT)
        assert len(got) == len(want) and got["p"].tobytes() == want["p"].tobytes() and got["n"].tobytes() == want["n"].tobytes()


_pose = []


def pose_of(cache):
    if not _pose:
        _pose.append(Pose(cache))
    return _pose[0]


def refusals(pose, tmp_path):
    """(what, arguments, exit code, a word of the one line it prints)"""
    c, out = pose.spec.config_path, ("--spp", "1", "--out", str(tmp_path / "never.exr"))
    return [
        ("a torn vertex", (c, "--pose", pose.torn, "--by-vertices") + out, 1, "tears vertex %d" % pose.idx[len(pose.idx) // 2, 1]),
        ("--by-vertices without --pose", (c, "--by-vertices") + out, 2, "--by-vertices needs --pose"),
        ("--recompute-normals without --by-vertices", (c, "--pose", pose.with_normals, "--recompute-normals") + out, 2, "--recompute-normals needs"),
        ("--recompute-normals alone", (c, "--recompute-normals") + out, 2, "--recompute-normals needs"),
    ]


def check_refusals(pose, tmp_path):
    for what, args, code, word in refusals(pose, tmp_path):
        got, log = run(*args)
        assert got == code and word in log, (what, got, log)
        assert not os.path.exists(str(tmp_path / "never.exr")), what
    # (positions tear whether or not the normals are passed on)
    got, log = run(pose.spec.config_path, "--pose", pose.torn, "--by-vertices", "--recompute-normals", "--out", str(tmp_path / "never.exr"))
    assert got == 1 and log.count("tears vertex") == 1 and not os.path.exists(str(tmp_path / "never.exr")), log


def test_cli_by_vertices(scene_cache, tmp_path):
    pose = pose_of(scene_cache)
    c, tail = pose.spec.config_path, ("--spp", "3", "--seed", "5")
    plain, by_vertices, computed = (str(tmp_path / name) for name in ("plain.exr", "by_vertices.exr", "computed.exr"))
    code, log = run(c, "--pose", pose.with_normals, *tail, "--out", plain)
    assert code == 0 and "triangles moved, refit" in log and "[PT]MESH:" not in log, log
    code, log = run(c, "--pose", pose.with_normals, "--by-vertices", *tail, "--out", by_vertices)
    assert code == 0, log
    valence = int(np.bincount(pose.idx.ravel()).max())
    line = "[PT]MESH: vertices %d triangles %d max_valence %d normals " % (len(pose.positions), len(pose.idx), valence)
    assert len(re.findall(r"^\[PT\]MESH:", log, re.M)) == 1 and line + "given\n" in log, log
    want = open(plain, "rb").read()
    assert open(by_vertices, "rb").read() == want
    code, log = run(c, "--pose", pose.without, "--by-vertices", "--recompute-normals", *tail, "--out", computed)
    assert code == 0 and line + "computed\n" in log, log
    assert open(computed, "rb").read() == want
    # the pose shows
    code, log = run(c, *tail, "--out", str(tmp_path / "rest.exr"))
    assert code == 0 and open(str(tmp_path / "rest.exr"), "rb").read() != want


def test_cli_by_vertices_under_a_policy(scene_cache, tmp_path):
    pose = pose_of(scene_cache)
    c, tail = pose.spec.config_path, ("--spp", "2", "--seed", "5", "--rebuild-above", "0", "--rebuild-method", "ploc")
    outs = []
    for road in ((), ("--by-vertices",)):
        outs.append(str(tmp_path / ("policy%d.exr" % len(road))))
        code, log = run(c, "--pose", pose.with_normals, *road, *tail, "--out", outs[-1])
        assert code == 0 and "pose policy" in log and "rebuilt" in log, log
    assert open(outs[0], "rb").read() == open(outs[1], "rb").read()


def test_cli_refusals(scene_cache, tmp_path):
    check_refusals(pose_of(scene_cache), tmp_path)
