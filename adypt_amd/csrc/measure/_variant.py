"""What the measurement variants share (NOT product code): the text edit every transform is made of, the one place that makes a variant tree and has
csrc/Makefile build from it, and the list of the named variants the tools and documents speak of.  A transform is   python k_x.py <device_dir>   ;
a variant is a copy of csrc/device with transforms applied in order, compiled by the Makefile's own rules (DEVICE= VARIANT= DEVFLAGS=).
tools/build_variant.sh, tools/build_counting_variants.sh, tools/trip_budget.py and tests/test_measure_variants.py all come through build().
    python _variant.py <name> [--transform measure/k_x.py]... [-D...]    = tools/build_variant.sh
    python _variant.py --counting                                        = tools/build_counting_variants.sh: the entries COUNTING of VARIANTS"""
import glob, os, shlex, shutil, subprocess, sys
MEASURE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.dirname(MEASURE)
K_PATH = "_ZN5adypt6k_pathILb0ELb0EEEvNS_12PathKernArgsE"  # k_path<false, false>: the kernel the measurements are about

B = "k_path_blocks.py"
# name: (transforms in order, environment of the transforms, -D flags of the compile)
VARIANTS = {
    # the seven counting configurations (tools/build_counting_variants.sh, tools/path_block_counts.py): wave entries per block, active lanes per block
    "blockcnt": ([B], {"ADYPT_BLOCKS_COUNT": "1"}, []),
    "shadecnt": ([B], {"ADYPT_BLOCKS_COUNT": "1", "ADYPT_BLOCKS_SET": "shade"}, []),
    "rarecnt": ([B], {"ADYPT_BLOCKS_COUNT": "1", "ADYPT_BLOCKS_SET": "rare"}, []),
    "lanes_trip": ([B], {"ADYPT_BLOCKS_COUNT": "1", "ADYPT_BLOCKS_LANES": "1", "ADYPT_BLOCKS_SET": "trip"}, []),
    "lanes_shade": ([B], {"ADYPT_BLOCKS_COUNT": "1", "ADYPT_BLOCKS_LANES": "1", "ADYPT_BLOCKS_SET": "shade"}, []),
    "lanes_rare": ([B], {"ADYPT_BLOCKS_COUNT": "1", "ADYPT_BLOCKS_LANES": "1", "ADYPT_BLOCKS_SET": "rare"}, []),
    "lanes_wait": ([B], {"ADYPT_BLOCKS_COUNT": "1", "ADYPT_BLOCKS_LANES": "1", "ADYPT_BLOCKS_SET": "wait"}, []),
    "marks": ([B], {"ADYPT_BLOCKS_COUNT": "0"}, []),  # marks only, no counters: the static counts of tools/trip_budget.py
    "timeline": (["k_path_timeline.py"], {}, []),
    "timeline_cap64": (["k_path_timeline.py", "k_path_init_cap.py"], {}, []),
    "cap64": (["k_path_init_cap.py"], {}, ["-DADYPT_PATH_INIT_CAP=64"]),
    "node128": (["k_node_stride128.py"], {}, []),
    "drain": (["k_path_drain_trace.py"], {}, []),
    "tailhist": (["k_path_tail_hist.py"], {}, []),
    "trionly": (["k_path_tri_only_trips.py"], {}, []),
    "trionly_absorbable": (["k_path_tri_only_trips.py"], {}, ["-DADYPT_COUNT_ABSORBABLE"]),
    "oneclass": (["k_path_one_material_class.py"], {}, []),
}
COUNTING = ["blockcnt", "shadecnt", "rarecnt", "lanes_trip", "lanes_shade", "lanes_rare", "lanes_wait"]


def edit(device_dir, file, pairs):
    """Replaces old by new in device_dir/file for every (old, new) of pairs; every old must be there exactly once."""
    p = os.path.join(device_dir, file)
    s = open(p).read()
    for old, new in pairs:
        if s.count(old) != 1:
            sys.exit("%s: %s: anchor found %d times instead of once: %r" % (os.path.basename(sys.argv[0]), file, s.count(old), old.strip("\n").split("\n")[0].strip()))
        s = s.replace(old, new)
    open(p, "w").write(s)


def run(cmd, env=None):
    """One step of a build.  What it prints goes to stderr; a failure raises with the end of it in the message, where a caller (or a test) shows it."""
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    sys.stderr.write(r.stdout)
    if r.returncode != 0:
        raise RuntimeError("%s: exit status %d\n%s" % (" ".join(cmd), r.returncode, r.stdout[-3000:]))


def make_tree(name, transforms, env={}):
    """csrc/.variant_<name> = csrc/device with the transforms (file names of this directory, or paths from the repository's root) applied in order.
    A sibling of device/, so the sources' ../../../include/*.h resolves as it does there; it must not exist yet.  Returns the directory relative to csrc."""
    rel = ".variant_" + name
    shutil.copytree(os.path.join(CSRC, "device"), os.path.join(CSRC, rel))
    for t in transforms:
        script = os.path.join(os.path.dirname(os.path.dirname(CSRC)), t) if os.sep in t else os.path.join(MEASURE, t)
        run([sys.executable, script, os.path.join(CSRC, rel)], env=dict(os.environ, **env))
    return rel


def discard(name):
    """Forgets a variant: its tree, and its objects and assembly under build/ (a library linked from them stays)."""
    shutil.rmtree(os.path.join(CSRC, ".variant_" + name), ignore_errors=True)
    for f in glob.glob(os.path.join(CSRC, "build", "*_%s.[os]" % name)):
        os.remove(f)


def build(name, transforms, env={}, flags=[], asm=False, jobs=8):
    """The variant's tree, then the Makefile on it: adypt_amd/libadypt_<name>.so (from build/*_<name>.o), or with asm only the device assembly
    build/tracer_<name>.s.  Returns what it built.  Without transforms the device sources themselves are compiled (a variant of flags only).
    A name's device objects are compiled anew on every call: neither the -D flags nor an earlier tree of that name are things make's timestamps know."""
    discard(name)
    dev = make_tree(name, transforms, env) if transforms else "device"
    out = os.path.join("build", "tracer_%s.s" % name) if asm else os.path.join("..", "libadypt_%s.so" % name)
    run(["make", "-s", "-C", CSRC, "-j%d" % jobs, "DEVICE=" + dev, "VARIANT=" + name, "DEVFLAGS=" + " ".join(map(shlex.quote, flags)), out])
    return os.path.normpath(os.path.join(CSRC, out))


if __name__ == "__main__":
    args = sys.argv[1:]
    if not args or args[0] in ("-h", "--help"):
        sys.exit(__doc__)
    todo = [(n,) + VARIANTS[n] for n in COUNTING] if args == ["--counting"] else [(args[0], [], {}, args[1:])]
    for name, transforms, env, flags in todo:
        while flags[:1] == ["--transform"]:
            transforms, flags = transforms + [flags[1]], flags[2:]
        try:
            build(name, transforms, env, flags)
        except RuntimeError as e:
            sys.exit("build of variant %s failed: %s" % (name, str(e).split("\n")[0]))
        print("built adypt_amd/libadypt_%s.so (%s)" % (name, " ".join(flags)))
