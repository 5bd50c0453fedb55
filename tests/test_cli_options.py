"""adypt_hip's command line where it ends before a device is asked for (csrc/cli/options.cpp: parse_options, check_options; the input loading of
csrc/cli/main.cpp).  No GPU.

CASES below are run against the built tool and compared, exit code and combined output byte for byte, with tests/golden/cli_refusals.json — recorded
from the tool as it was before its options became one record and one table (the commit is named in the file), so the reference is that tool's
behaviour and not this one's.  `python tests/test_cli_options.py EXE` records the file from EXE.  The usage text is the one thing that may differ: it
is held against the option names in the sources instead.  Below that: what the command line refuses, as the -m gpu tests of each feature asserted it
beside their renders, here where it runs without a GPU."""
import glob
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from adypt_amd import _native as N  # noqa: E402
from adypt_amd import scenes  # noqa: E402

EXE = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")
FIXTURE = os.path.join(ROOT, "tests", "golden", "cli_refusals.json")
CLI_SOURCES = os.path.join(ROOT, "adypt_amd", "csrc", "cli")

C, OBJ, OTHER, OTHER_C = "{config}", "{obj}", "{other_obj}", "{other_config}"
D = ("--denoise", "{tmp}/d.exr")
TEMPORAL = D + ("--history-cap", "16")
TAIL = ("--spp", "1", "--out", "{tmp}/o.exr")
VALUE_OPTIONS = ("--spp", "--out", "--preview", "--primary", "--seed", "--device", "--devices", "--save-every", "--noise", "--min-spp", "--check-every", "--noise-out", "--spp-out",
                 "--denoise", "--denoise-levels", "--history-from", "--history-out", "--history-cap", "--rectify-out", "--rectify-radius", "--rectify-gamma", "--guides-out", "--pose",
                 "--part-matrices", "--morph-target", "--morph-weights", "--rebuild-above", "--rebuild-method", "--build", "--ploc-radius", "--split-budget")
CASES = [
    (),  # the usage
    # what does not go together, in the order the tool looks
    (C, "--build", "gpu", "--rebuild"),
    (C, "--rebuild-method", "sah"),
    (C, "--rebuild-method", ""),
    (C, "--build", "gpu", "--rebuild-method", "sah"),
    (C, "--rebuild", "--split-budget", "0.3"),
    (C, "--split-budget", "0.3"),
    (C, "--build", "gpu", "--rebuild-method", "linear", "--split-budget", "0.3"),
    (C, "--pose", OBJ, "--part-matrices", "{tmp}/parts.txt"),
    (C, "--morph-target", OBJ),
    (C, "--morph-weights", "0.5"),
    (C, "--morph-target", OBJ, "--morph-weights", "0.5,0.25"),
    (C, "--morph-target", OBJ, "--morph-target", OBJ, "--morph-weights", "0.5"),
    (C, "--morph-target", OBJ, "--morph-weights", "0.5", "--pose", OBJ),
    (C, "--morph-target", OBJ, "--morph-weights", "1,2", "--morph-weights", "3", "--pose", OBJ),  # the last list counts
    (C, "--rebuild-above", "1.4"),
    (C, "--pose", OBJ, "--rebuild-above", "1.4", "--rebuild"),
    (C, "--part-matrices", "{tmp}/parts.txt", "--rebuild-above", "0", "--rebuild", "--rebuild-method", "ploc"),
    (C, "--pose", OBJ, "--rebuild-above", "1.4", "--split-budget", "0.3"),
    (C, "--noise-out", "{tmp}/n.exr"),
    (C, "--noise", "0.1", "--primary", "0"),
    (C, "--noise", "0.1", "--spp", "1"),
    (C, "--noise", "0.1", "--check-every", "0"),
    (C, "--adaptive"),
    (C, "--noise", "0.1", "--adaptive", "--save-every", "4"),
    (C, "--spp-out", "{tmp}/s.exr"),
    (C, "--noise", "0.1", "--spp-out", "{tmp}/s.exr"),
    (C,) + D + ("--spp", "1"),
    (C,) + D + ("--primary", "0"),
    (C,) + D + ("--denoise-levels", "7"),
    (C,) + D + ("--denoise-levels", "0"),
    (C, "--history-from", C),
    (C, "--history-cap", "16"),
    (C, "--history-out", "{tmp}/l.exr"),
    (C,) + TEMPORAL + ("--rectify-gamma", "1"),
    (C,) + TEMPORAL + ("--rectify-radius", "2"),
    (C,) + TEMPORAL + ("--rectify-out", "{tmp}/k.exr"),
    (C,) + TEMPORAL + ("--rectify-out", ""),
    (C,) + D + ("--rectify",),
    (C, "--rectify"),
    (C,) + D + ("--follow-motion",),
    (C, "--follow-motion"),
    (C, "--build", "cpu"),
    # the bounded numbers
    *[(C, option, bad) for option, beyond in (("--history-cap", ("0", "4e38", "1e-400")), ("--rectify-radius", ("0", "4", "2.0", "99999999999999999999")), ("--rectify-gamma", ("4e38", "-0.5")),
                                              ("--rebuild-above", ("1e999", "-1e-9")))
      for bad in ("nan", "inf", "-inf", "-1", "1x", "x", "", " ") + beyond],
    # the lists
    *[(C, "--devices", bad) for bad in ("", "0,x", "x", "-1", ",", "0,,1", "0 1", "1.5")],
    (C, "--devices", "0,", "--rebuild-method", "sah"),  # (a trailing comma passes)
    (C, "--devices", "x", "--devices", "0", "--rebuild-method", "sah"),
    *[(C, "--morph-target", OBJ, "--morph-weights", bad) for bad in ("", "0.5,", "half", ",", "0.5,,1", "0.5x", "0.5 1")],
    (C, "--morph-target", OBJ, "--morph-weights", "nan", "--pose", OBJ),
    # an option that takes a value, given last without one; words that are no option
    *[(C, option) for option in VALUE_OPTIONS],
    (C, "--pose", OBJ, "--rebuild-above"),
    (C, "--frobnicate"),
    (C, "extra"),
    (C, "-spp", "4"),
    (C, "--spp", "4", "--"),
    # two rules broken at once: argv order while parsing, then the order of the checks
    (C, "--build", "gpu", "--rebuild", "--rebuild-method", "sah"),
    (C, "--rebuild-method", "sah", "--split-budget", "0.3"),
    (C, "--pose", OBJ, "--part-matrices", "{tmp}/parts.txt", "--morph-target", OBJ),
    (C, "--rebuild-above", "1.4", "--rebuild"),
    (C, "--noise-out", "{tmp}/n.exr", "--adaptive"),
    (C,) + D + ("--spp", "1", "--denoise-levels", "9"),
    (C, "--history-cap", "16", "--rectify-gamma", "1"),
    (C, "--rectify", "--follow-motion"),
    (C, "--follow-motion", "--rectify"),
    (C, "--spp-out", "{tmp}/s.exr") + D + ("--spp", "1"),
    (C, "--rebuild", "--build", "gpu", "--history-cap", "nan"),
    (C, "--history-cap", "nan", "--rectify-radius", "9"),
    (C, "--rectify-radius", "9", "--history-cap", "nan"),
    (C, "--frobnicate", "--history-cap", "nan"),
    (C, "--history-cap", "nan", "--frobnicate"),
    (C, "--rebuild-method", "sah", "--spp"),
    ("{tmp}/missing.config", "--rebuild-method", "sah"),
    # the inputs: exit 1, still before any device
    ("{tmp}/missing.config",) + TAIL,
    (C, "--pose", OTHER) + TAIL,
    (C, "--pose", "{tmp}/missing.obj") + TAIL,
    (C, "--morph-target", OTHER, "--morph-weights", "1") + TAIL,
    (C, "--morph-target", OBJ, "--morph-target", OTHER, "--morph-weights", "1,1") + TAIL,
    (C, "--morph-target", "{tmp}/missing.obj", "--morph-weights", "1") + TAIL,
    (C, "--part-matrices", "{tmp}/missing.txt") + TAIL,
    (C, "--part-matrices", "{tmp}/short_line.txt") + TAIL,
    (C, "--part-matrices", "{tmp}/junk_after.txt") + TAIL,
    (C, "--part-matrices", "{tmp}/no_such_part.txt") + TAIL,
    (C,) + D + ("--history-from", "{tmp}/wider.config", "--spp", "2", "--out", "{tmp}/o.exr"),
    (C,) + D + ("--history-from", C, "--history-from", OTHER_C, "--spp", "2", "--out", "{tmp}/o.exr"),
    (C,) + D + ("--history-from", "{tmp}/missing.config", "--spp", "2", "--out", "{tmp}/o.exr"),
    (C, "--pose", OTHER, "--build", "gpu") + TAIL,
]


class Inputs:
    """tiny0 and tiny2 at 64x36 and the small files the cases name, all under one directory"""

    def __init__(self, tmp):
        self.tmp = tmp
        scene = scenes.make_scene("tiny0", tmp, width=64, height=36)
        other = scenes.make_scene("tiny2", tmp, width=64, height=36)
        self.words = {"{config}": scene.config_path, "{obj}": scene.obj_path, "{other_obj}": other.obj_path, "{other_config}": other.config_path}
        identity = "1 0 0 0 0 1 0 0 0 0 1 0"
        for name, text in (("parts.txt", "# one part, where it is\n\n0 %s\n" % identity), ("short_line.txt", "0 %s\n1 1 0 0 0\n" % identity),
                           ("junk_after.txt", "0 %s and more\n" % identity), ("no_such_part.txt", "0 %s\n9999 %s\n" % (identity, identity))):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        wider = json.load(open(scene.config_path))
        wider["width"] += 4
        json.dump(wider, open(os.path.join(tmp, "wider.config"), "w"), indent=4)

    def run(self, exe, case):
        """exit code and combined output of one case, the directory's and the tool's names taken out of the output"""
        args = [self.words.get(a, a).replace("{tmp}", self.tmp) for a in case]
        r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
        return r.returncode, r.stdout.decode().replace(self.tmp, "{tmp}").replace(exe, "{exe}")

    def state(self):
        """every file of the directory with its bytes: no case may write one (an image, a .part, a .bvh cache) or touch one (the config's write-back)"""
        return {name: open(os.path.join(self.tmp, name), "rb").read() for name in sorted(os.listdir(self.tmp))}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return Inputs(str(tmp_path_factory.mktemp("cli_options")))


def test_refusals_are_what_they_were(inputs):
    recorded = json.load(open(FIXTURE))
    assert [r["args"] for r in recorded["cases"]] == [list(c) for c in CASES], "tests/golden/cli_refusals.json was recorded for another list of cases"
    before = inputs.state()
    for case, want in zip(CASES, recorded["cases"]):
        code, text = inputs.run(EXE, case)
        assert code in (1, 2) and code == want["code"], (case, code, text)
        if case:  # (the usage: test_usage_names_every_option)
            assert text == want["output"], (case, text, want["output"])
    assert inputs.state() == before, "a refused command line wrote a file"


def test_usage_names_every_option(inputs):
    """every "--option" literal of the sources (the table's names among them) is in the usage text, --test-hooks aside: it is for the tests"""
    names = set()
    for path in glob.glob(os.path.join(CLI_SOURCES, "*.[ch]pp")):
        names |= set(re.findall(r'"(--[a-z][a-z0-9-]*)"', open(path).read()))
    assert {"--spp", "--morph-target", "--morph-weights", "--test-hooks"} <= names and set(VALUE_OPTIONS) <= names, sorted(names)
    code, usage = inputs.run(EXE, ())
    assert code == 2 and usage.startswith("usage: ") and usage.count("\n") == 1, usage
    missing = [n for n in sorted(names - {"--test-hooks"}) if not re.search(re.escape(n) + r"(?![a-z0-9-])", usage)]
    assert not missing and "--test-hooks" not in usage, (missing, usage)
    assert "--morph-target FILE.obj" in usage and "--morph-weights w0,w1,..." in usage


# ---- the refusals the feature tests asserted beside their renders (tests/test_gpu_*.py), with their assertions ----
@pytest.fixture()
def cli(scene_cache, tmp_path):
    """the tool on tiny0 64x36 with an --out, as the feature tests call it: cli(*args) -> (exit code, output); cli.out must not appear"""
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    copy = str(tmp_path / "main.config")  # (the tool writes its config back on exit)
    json.dump(json.load(open(spec.config_path)), open(copy, "w"), indent=4)
    out = str(tmp_path / "o.exr")

    def run(*args, tail=("--spp", "4")):
        r = subprocess.run([EXE, copy, "--out", out, "--seed", "3"] + list(tail) + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        return r.returncode, (r.stdout + r.stderr).decode()
    run.spec, run.config, run.out, run.tmp = spec, copy, out, tmp_path
    yield run
    assert not os.path.exists(out)


def test_rectify_options(cli):
    # the rectify options need --rectify, --rectify needs a temporal --denoise call, and parameters inside their ranges
    d_exr = str(cli.tmp / "d.exr")
    for bad in (("--denoise", d_exr, "--rectify"), ("--rectify",), ("--denoise", d_exr, "--history-cap", "16", "--rectify-gamma", "1"),
                ("--denoise", d_exr, "--history-cap", "16", "--rectify", "--rectify-radius", "4"), ("--denoise", d_exr, "--history-cap", "16", "--rectify", "--rectify-gamma", "nan")):
        code, text = cli(*bad)
        assert code == 2 and "--rectify" in text, text


def test_follow_motion_needs_a_temporal_call(cli):
    d_exr = str(cli.tmp / "d.exr")
    for bad in (("--follow-motion",), ("--denoise", d_exr, "--follow-motion")):
        code, text = cli(*bad)
        assert code == 2 and "--follow-motion" in text, text


def test_denoise_options(cli):
    # refused before anything is loaded
    d_exr = str(cli.tmp / "d.exr")
    for bad in (("--spp", "1", "--denoise", d_exr), ("--primary", "0", "--denoise", d_exr), ("--spp", "8", "--denoise", d_exr, "--denoise-levels", "7")):
        code, text = cli(*bad, tail=())
        assert code == 2 and "--denoise" in text, text


def test_history_options(cli):
    d_exr = str(cli.tmp / "d.exr")
    main = json.load(open(cli.config))
    # a config of another size is refused
    other = json.loads(json.dumps(main))
    other["width"] = main["width"] + 4
    wrong = str(cli.tmp / "wrong.config")
    json.dump(other, open(wrong, "w"), indent=4)
    code, text = cli("--denoise", d_exr, "--history-from", wrong)
    assert code == 1 and "another size" in text, text[-2000:]
    # the history options need --denoise, and a cap that is a positive finite number
    for bad in (("--history-from", cli.config), ("--denoise", d_exr, "--history-cap", "0"), ("--denoise", d_exr, "--history-cap", "nan")):
        code, text = cli(*bad)
        assert code == 2 and "--history" in text, text


def test_morph_options(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    other = scenes.make_scene("tiny2", scene_cache, width=64, height=36)
    out = str(tmp_path / "o.exr")
    tail = ("--spp", "1", "--out", out)

    def run(*args):
        r = subprocess.run([EXE] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        return r.returncode, r.stdout.decode()
    for args, word in ((("--morph-target", spec.obj_path), "go together"),
                       (("--morph-weights", "0.5"), "go together"),
                       (("--morph-target", spec.obj_path, "--morph-weights", "0.5,0.25"), "2 weights for 1"),
                       (("--morph-target", spec.obj_path, "--morph-target", spec.obj_path, "--morph-weights", "0.5"), "1 weights for 2"),
                       (("--morph-target", spec.obj_path, "--morph-weights", "0.5", "--pose", spec.obj_path), "--pose"),
                       (("--morph-target", spec.obj_path, "--morph-weights", "0.5,"), "bad --morph-weights"),
                       (("--morph-target", spec.obj_path, "--morph-weights", "half"), "bad --morph-weights")):
        code, log = run(spec.config_path, *args, *tail)
        assert code == 2 and word in log, (args, log)
    # a target with another triangle count: an error, found before any device is asked for
    code, log = run(spec.config_path, "--morph-target", other.obj_path, "--morph-weights", "1", *tail)
    assert code == 1 and "has 5 triangles, the scene has 554" in log, log
    code, log = run(spec.config_path, "--morph-target", str(tmp_path / "missing.obj"), "--morph-weights", "1", *tail)
    assert code == 1 and "Unable to load morph target" in log, log
    assert not os.path.exists(out)


def test_part_matrices_options(scene_cache, tmp_path):
    import numpy as np
    from adypt_amd import api
    from oracle import oracle_py as O
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    scene = api.Scene()
    assert scene.LoadFromFile(spec.obj_path)
    matid = np.array(scene.triangles).view(O.TRI_DT)["matid"]
    n_mats = len(np.ascontiguousarray(scene.materials).view(O.MAT_DT).reshape(-1))
    n_parts = n_mats + (1 if ((matid < 0) | (matid >= n_mats)).any() else 0)
    assert n_parts >= 2
    out = str(tmp_path / "pose.exr")
    table = str(tmp_path / "parts.txt")
    with open(table, "w") as f:
        f.write("# part m00 m01 m02 m03 m10 ... m23\n\n0 1 0 0 0 0 1 0 0 0 0 1 0\n%d 1 0 0 0.5 0 1 0 0 0 0 1 0\n" % (n_parts - 1))
    # two ways to move the scene at once
    r = subprocess.run([EXE, spec.config_path, "--part-matrices", table, "--pose", spec.obj_path, "--spp", "1", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 2 and "--part-matrices" in r.stdout.decode(), r.stdout.decode()
    # a part the scene does not have
    with open(table, "a") as f:
        f.write("%d 1 0 0 0 0 1 0 0 0 0 1 0\n" % n_parts)
    r = subprocess.run([EXE, spec.config_path, "--part-matrices", table, "--spp", "1", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 1 and "line 5" in r.stdout.decode(), r.stdout.decode()
    assert not os.path.exists(out)


def test_devices_rebuild_method_and_split_budget(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    out = str(tmp_path / "o.exr")
    r = subprocess.run([EXE, spec.config_path, "--devices", "0,x"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 2 and b"bad --devices" in r.stdout
    r = subprocess.run([EXE, spec.config_path, "--rebuild-method", "sah"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 2
    r = subprocess.run([EXE, spec.config_path, "--rebuild", "--split-budget", "0.3", "--spp", "1", "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 2, r.stdout.decode()
    assert not os.path.exists(out) and not os.path.exists("result.exr")


def record(exe):
    """tests/golden/cli_refusals.json from the tool at exe"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        inputs = Inputs(tmp)
        before = inputs.state()
        cases = [dict(zip(("code", "output"), inputs.run(exe, case)), args=list(case)) for case in CASES]
        assert inputs.state() == before
    commit = subprocess.run(["git", "-C", ROOT, "log", "-1", "--format=%h %s"], stdout=subprocess.PIPE).stdout.decode().strip()
    note = "exit code and combined output of adypt_hip for tests/test_cli_options.py's CASES, as built from the commit named here; {tmp} is the directory the test works in"
    with open(FIXTURE, "w") as f:
        json.dump({"note": note, "recorded_from": commit, "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    record(sys.argv[1])
