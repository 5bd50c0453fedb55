"""-m gpu: k_chain_start<false | true> and k_chain_step<false | true> (csrc/device/denoise_kernels.hpp) ONE LAUNCH AT A TIME on the hand-made inputs of
tests/chain_edge_inputs.py, through adypt_amd/libadypt_probe.so (tests/probe.py), which launches each with the launch shape the product uses.  Through
the product the two kernels only ever see what a traversal of a well-formed scene hands them; here they see pixel words that are no pixel, hit words
and material ids outside their tables, a count above a segment's capacity, every illum, ior 0 and NaN, zero and NaN normals, and every pattern of
followed lanes the wave-wide append can meet.

The conventions are tests/test_gpu_denoise_probes.py's: probe.same against the numpy truths (tests/specular_truth.py start and step, tests/virtual_truth.py
for the lengths) with no tolerance; every output pre-filled with a sentinel that written words must have lost and unwritten words must still hold; every
case proven to reach its branch from its inputs or from the truth's side.  A queue is compared as a set per segment keyed by the pixel word — waves reach
the atomic in any order — and one wave's rays must sit in consecutive slots in lane order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import chain_edge_inputs as CE  # noqa: E402
from tests import probe as P  # noqa: E402
from tests.test_gpu_denoise_probes import check  # noqa: E402

F = np.float32
SCENE = CE.scene()


def same_where(got, want, mask, what):
    """the words of `got` under `mask` are the truth's and have lost the sentinel; all others still hold what they held going in (`want` there)"""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    mask = np.broadcast_to(mask, got.shape)
    ok = P.same(got, want)
    assert ok.all(), "%s: %d words differ, the first at %s: device %r, truth %r" % (what, int((~ok).sum()), np.argwhere(~ok)[0].tolist(), got[tuple(np.argwhere(~ok)[0])],
                                                                                 want[tuple(np.argwhere(~ok)[0])])
    assert not P.unwritten(got[mask]).any(), what + ": a word the truth says is written still holds the sentinel"


def check_queue(got, rays, has, segment_of, wave_of, seg_cap, what):
    """got: the probe's dict (o, d, count, count_words); rays = (o, d) per source index and `has`: which source indices append a ray; segment_of: the
    segment of every source index; wave_of(pixel word) -> (wave, lane)."""
    segments = len(got["count"])
    assert (got["count_words"][:, 1:] == 0).all(), what + ": a counter word that belongs to no segment changed"
    for s in range(segments):
        src = np.flatnonzero(has & (segment_of == s))
        assert int(got["count"][s]) == len(src), "%s: segment %d counts %d rays, the truth %d" % (what, s, int(got["count"][s]), len(src))
        n = min(len(src), seg_cap)
        o, d = got["o"][s], got["d"][s]
        assert P.unwritten(o[n:]).all() and P.unwritten(d[n:]).all(), "%s: segment %d: a slot past the count was written" % (what, s)
        assert not P.unwritten(o[:n]).any() and not P.unwritten(d[:n]).any(), "%s: segment %d: a slot below the count holds the sentinel" % (what, s)
        words = CE.as_word(d[:n, 3])
        by_word = {int(CE.as_word(rays[1][i, 3:4])[0]): i for i in src}
        assert len(set(words.tolist())) == n and set(words.tolist()) <= set(by_word), "%s: segment %d holds pixel words the truth does not" % (what, s)
        if n == len(src):
            assert set(words.tolist()) == set(by_word)
        pick = np.array([by_word[int(w)] for w in words], np.int64)
        if n:
            assert P.same(o[:n], rays[0][pick]).all() and P.same(d[:n], rays[1][pick]).all(), "%s: segment %d: a ray differs from the truth's" % (what, s)
        assert CE.wave_order_ok(words, wave_of), "%s: segment %d: a wave's rays do not sit in consecutive slots in lane order" % (what, s)


# ---- k_chain_start ----
@pytest.mark.parametrize("unfold", [False, True], ids=["plain", "unfold"])
@pytest.mark.parametrize("segments", CE.START_SEGMENTS)
@pytest.mark.parametrize("pattern", CE.START_PATTERNS)
@pytest.mark.parametrize("n_blocks", [1, 2, 3])
@pytest.mark.parametrize("picture", list(CE.START_PICTURES))
def test_start(picture, n_blocks, pattern, segments, unfold):
    case = CE.start_case(picture, n_blocks, pattern)
    t = CE.start_truth(SCENE, case, unfold)
    assert CE.start_reach(case, t), "the case does not reach what it is named after"
    n_px, go = case["n_px"], t["go"]
    seg_cap = ((n_px // 256 + segments - 1) // segments) * 256  # the most rays a segment is given, as the product sizes it
    got = P.chain_start(unfold, SCENE.device, case["albedo"], case["normal"], case["position"], case["hits"], case["blocks"], case["w"], case["h"], CE.ORIGIN, CE.TMIN, case["K"],
                        segments, seg_cap)
    what = "%s, %d blocks, %s, %d segments, unfold %s: " % (picture, n_blocks, pattern, segments, unfold)
    for k in ("albedo", "normal", "position"):
        assert P.same(got[k], case[k]).all(), what + "the start changed the %s guide" % k
    want_hits = case["hits"].copy()
    want_hits[:, 3] = t["hits_w"]  # (a followed pixel's, and a pixel's outside the picture, is untouched)
    ok = P.same(got["hits"], want_hits)
    assert ok.all(), "%sthe class words, or another word of the hits: %d differ, the first at %s" % (what, int((~ok).sum()), np.argwhere(~ok)[0].tolist())
    same_where(got["state"], t["state"], go[:, None, None], what + "the state")
    assert P.unwritten(got["state"][~go]).all()
    assert got["counts"] == dict(rays=int(go.sum()), followed=int(go.sum()), escaped=0, truncated=0), what + str(got["counts"])
    check_queue(got, (t["o"], t["d"]), go, (np.arange(n_px) // 256) % segments, lambda L: (L // 64, L % 64), seg_cap, what)


@pytest.mark.parametrize("unfold", [False, True], ids=["plain", "unfold"])
def test_start_overflow(unfold):
    """One wave of 64 followed pixels into a segment of 40 slots: the count reads 64, slots 0..39 hold lanes 0..39, the guard drops the rest and the other
    segment keeps the sentinel — nothing is written outside an array."""
    case = CE.overflow_case()
    t = CE.start_truth(SCENE, case, unfold)
    assert CE.start_reach(case, t) and t["go"][:64].all() and t["go"].sum() == 64
    got = P.chain_start(unfold, SCENE.device, case["albedo"], case["normal"], case["position"], case["hits"], case["blocks"], case["w"], case["h"], CE.ORIGIN, CE.TMIN, case["K"], 2, 40)
    assert got["count"].tolist() == [64, 0] and (got["count_words"][:, 1:] == 0).all()
    assert CE.as_word(got["d"][0, :, 3]).tolist() == list(range(40)), "slots 0..39 hold lanes 0..39"
    assert P.same(got["o"][0], t["o"][:40]).all() and P.same(got["d"][0], t["d"][:40]).all()
    assert P.unwritten(got["o"][1]).all() and P.unwritten(got["d"][1]).all(), "segment 1 keeps the sentinel"
    same_where(got["state"], t["state"], t["go"][:, None, None], "the state")
    assert got["counts"] == dict(rays=64, followed=64, escaped=0, truncated=0)


# ---- k_chain_step ----
@pytest.mark.parametrize("unfold", [False, True], ids=["plain", "unfold"])
@pytest.mark.parametrize("name", list(CE.STEP_COUNTS))
def test_step(name, unfold):
    case = CE.step_case(name)
    t = CE.step_truth(SCENE, case, unfold)
    assert CE.step_reach(SCENE, case, t, unfold), "the case does not reach what it is named after"
    got = P.chain_step(unfold, SCENE.device, case["albedo"], case["normal"], case["position"], case["hits"], case["state"], case["queue"], CE.STEP_K, CE.TMIN,
                       virt=case["virt"] if unfold else None, origin=CE.ORIGIN if unfold else None)
    what = "%s, unfold %s: " % (name, unfold)
    for k in ("albedo", "normal", "position", "hits", "state") + (("virt",) if unfold else ()):
        ok = P.same(got[k], t[k])
        assert ok.all(), "%s%s: %d words differ, the first at %s (a pixel that is not named by a consumed ray keeps every word)" % (what, k, int((~ok).sum()), np.argwhere(~ok)[0].tolist())
    assert got["counts"] == dict(rays=int(t["go"].sum()), followed=0, escaped=t["escaped"], truncated=t["truncated"]), what + str(got["counts"])
    n_slots = CE.STEP_SEGMENTS * CE.STEP_SEG_CAP
    slot_of = {int(w): i for i, w in enumerate(case["word"]) if t["go"][i]}
    check_queue(got, t["rays"], t["go"], np.arange(n_slots) // CE.STEP_SEG_CAP, lambda L: divmod(slot_of[L] % CE.STEP_SEG_CAP, 64), CE.STEP_SEG_CAP, what)
