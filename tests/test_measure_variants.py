"""Every named measurement variant (adypt_amd/csrc/measure/_variant.py: VARIANTS) must still apply to the device sources as they are and compile
(CPU only).  The transforms are text patches anchored in path.hpp / traverse_trip.inc / shade.hpp: an edit of those files that moves an anchor kills a
transform silently, and the instruction-issue roofline of bench.py is built from the counting variants.  For each variant: a fresh copy of csrc/device,
its transforms in order (each anchor found exactly once, or the transform exits non-zero), then tracer.hip compiled device-only to gfx950 assembly
by the Makefile's own asm rule — the product's flags plus the variant's -D flags — and the kernel the measurements are about, k_path<false, false>, is in it.
Every variant gets the full -S compile (no -fsyntax-only short cut); they are compiled once, together, eight at a time."""
import concurrent.futures
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adypt_amd", "csrc", "measure"))
import _variant  # noqa: E402


def _build(name):
    # (a name of the test's own: tools/trip_budget.py, run by another test, builds `marks` at build/tracer_marks.s)
    try:
        return _variant.build("test_" + name, *_variant.VARIANTS[name], asm=True, jobs=1), None
    except RuntimeError as e:
        return None, str(e)


@pytest.fixture(scope="module")
def built():
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        yield dict(zip(_variant.VARIANTS, pool.map(_build, _variant.VARIANTS)))
    for name in _variant.VARIANTS:  # (3 MB of assembly and a source tree per variant: not left behind)
        _variant.discard("test_" + name)


def test_the_documented_variants_are_listed():
    assert set(_variant.COUNTING) <= set(_variant.VARIANTS) and len(_variant.COUNTING) == 7
    for name, (transforms, env, flags) in _variant.VARIANTS.items():
        assert transforms and all(os.path.isfile(os.path.join(_variant.MEASURE, t)) for t in transforms), name
        assert all(f.startswith("-D") for f in flags), name
    # no transform is left outside the list: one that nothing names is one that nothing checks
    have = {f for f in os.listdir(_variant.MEASURE) if f.startswith("k_") and f.endswith(".py")}
    assert have == {t for transforms, _, _ in _variant.VARIANTS.values() for t in transforms}


@pytest.mark.parametrize("name", list(_variant.VARIANTS))
def test_variant_applies_and_compiles(built, name):
    asm, err = built[name]
    assert err is None, err  # a transform whose anchor moved (it names the anchor), or a compile error
    text = open(asm).read()
    assert "\n" + _variant.K_PATH + ":" in text and ".amdhsa_kernel " + _variant.K_PATH in text


def test_a_name_built_again_is_compiled_again():
    """A sweep builds one name over and over with other -D flags (path.hpp: ADYPT_PATH_SLOTS), or a name once made from a transform again without
    it: every call must compile what it was given, whatever is left under build/ from the call before."""
    def k_path(asm):
        text = open(asm).read()
        return text[text.index("\n" + _variant.K_PATH + ":"):text.index(".amdhsa_kernel " + _variant.K_PATH)]
    try:
        capped = k_path(_variant.build("test_again", ["k_path_init_cap.py"], asm=True, jobs=1))
        slots320 = k_path(_variant.build("test_again", [], flags=["-DADYPT_PATH_SLOTS=320"], asm=True, jobs=1))
        slots256 = k_path(_variant.build("test_again", [], flags=["-DADYPT_PATH_SLOTS=256"], asm=True, jobs=1))
        assert capped != slots320 and slots320 != slots256 and slots256 != capped
    finally:
        _variant.discard("test_again")
