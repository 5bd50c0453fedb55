"""adypt_hip --history-samples where the command line ends before a device is asked for (csrc/cli/options.cpp): the option record, the values it
takes, and the combinations that exit 2.  No GPU."""
import os
import subprocess

from adypt_amd import _native as N
from adypt_amd import scenes

EXE = os.path.join(os.path.dirname(N.LIB_PATH), "adypt_hip")


def test_history_samples_option_record(scene_cache, tmp_path):
    spec = scenes.make_scene("tiny0", scene_cache, width=64, height=36)
    out, d_exr, r_exr, p_exr = (str(tmp_path / f) for f in ("o.exr", "d.exr", "reach.exr", "want.exr"))
    missing = str(tmp_path / "missing.config")

    def cli(*args, spp="8"):
        r = subprocess.run([EXE, spec.config_path] + list(args) + ["--spp", spp, "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=str(tmp_path))
        return r.returncode, r.stdout.decode()
    temporal = ("--denoise", d_exr, "--history-cap", "16")
    plan = temporal + ("--history-samples", "16")
    # it needs a temporal --denoise call
    for args in (("--history-samples", "16"), ("--denoise", d_exr, "--history-samples", "16")):
        code, text = cli(*args)
        assert code == 2 and "--history-samples needs a temporal --denoise call" in text, (args, text)
    # what it does not combine with
    for extra in (("--noise", "0.05"), ("--noise", "0.05", "--adaptive"), ("--save-every", "2")):
        code, text = cli(*plan, *extra)
        assert code == 2 and "--history-samples plans the samples itself" in text, (extra, text)
    for extra in (("--rectify",), ("--follow-specular", "2")):
        code, text = cli(*plan, *extra)
        assert code == 2 and "--history-samples does not combine with --rectify or --follow-specular" in text, (extra, text)
    code, text = cli(*plan, "--denoise-moments", spp="1")
    assert code == 2 and "--history-samples needs --spp >= 2" in text, text
    # its companions need it
    for extra in (("--history-step", "2"), ("--history-tolerance", "0"), ("--reach-out", r_exr), ("--plan-out", p_exr)):
        code, text = cli(*temporal, *extra)
        assert code == 2 and "need --history-samples T" in text, (extra, text)
    # the values
    for args, word in ((("--history-samples", "0"), "--history-samples takes"), (("--history-samples", "1048577"), "--history-samples takes"), (("--history-samples", "2.5"), "--history-samples takes"),
                       (("--history-samples", "16", "--history-step", "0"), "--history-step takes"), (("--history-samples", "16", "--history-tolerance", "1000"), "--history-tolerance takes"),
                       (("--history-samples", "16", "--history-tolerance", "-1"), "--history-tolerance takes")):
        code, text = cli(*temporal, *args)
        assert code == 2 and word in text, (args, text)
    code, text = cli(*temporal, "--history-samples")  # (the value is missing: `--spp` is taken for it)
    assert code == 2, text
    # accepted: the tool goes on and fails on the config it is given
    for extra in ((), ("--follow-motion",), ("--denoise-moments",), ("--history-step", "2", "--history-tolerance", "0", "--reach-out", r_exr, "--plan-out", p_exr),
                  ("--history-samples", "1048576")):
        code, text = cli(*plan, "--history-from", missing, *extra)
        assert code == 1 and "Invalid instance" in text and "--history-samples" not in text, (extra, code, text)
    assert not os.listdir(str(tmp_path)), "a refused command line wrote a file"
    usage = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    assert "[--history-samples T [--history-step S] [--history-tolerance P] [--reach-out reach.exr] [--plan-out want.exr]]" in usage
