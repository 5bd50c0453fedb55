"""-m gpu: adaptive sampling (include/adypt_hip.h adypt_trace_adaptive; csrc/device/active_blocks.hpp).  A block that stops at n spp holds exactly the
pixels of the uniform image at n spp, so the truth is exact and computed in this process from the CPU oracle's per-frame samples (tests/noise_truth.py),
never taken from the library: the table `block mean noise at every check` from the uniform sample sequence, the schedule spp_b from the table, the
expected image = images[spp_b - 1] per block, the moments = T.moments(samples[:spp_b]) per block, the per-pixel noise with n = spp_b.  Image,
moments, per-pixel noise, ReadBlockSPP and GetSPP bit for bit; block sums and image numbers within the suite's 2^-40 relative (tests/test_gpu_noise.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import noise_truth as T  # noqa: E402
from tests.helpers import bits, oracle_scene_from_instance  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "adypt_amd", "adypt_hip")
REL = 2.0 ** -40
SEED = 31
B = 32

#         scene      w    h  life sub  every min cap  nominal target (the test's own target is the geometric mean of the two table entries around it)
TINY0 = ("tiny0", 100, 75, 4, 1, 8, 8, 64, 0.1)      # 4 x 3 blocks, partial ones at the right and bottom edge; six blocks without noise
SIBENIK = ("sibenik", 160, 90, 3, 1, 8, 8, 48, 0.435)  # 15 blocks; checks fall in the middle of tmpLifetime groups
SMALL = ("tiny0", 96, 64, 4, 1, 6, 6, 48, 0.1)       # mid-group set changes with only 6 blocks
_truth_cache = {}


def _instance(cache, case):
    name, w, h, life, sub = case[:5]
    spec = scenes.make_scene(name, cache, width=w, height=h, pt={"tmpLifetime": life, "maxBounce": 6, "subpixel": sub})
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=SEED), api.InstanceConfig.last_error()
    return inst, spec


def _truth(inst, case, sobol_matrices, sun=False):
    """(samples of every frame, the oracle's image after every frame) up to the case's cap, computed once per session and never written to."""
    key = case + (sun,)
    if key not in _truth_cache:
        n = case[7]
        c = inst.m_config.c
        osc, P, shift = oracle_scene_from_instance(inst), T.oracle_params(c, sun), O.shift_bytes(SEED, c.width, c.height)
        samples = T.frame_samples(osc, P, shift, sobol_matrices, n)
        state, images = O.PathTracerState(c.width, c.height), []
        for _ in range(n):
            O.pt_frames(osc, P, shift, sobol_matrices, state, 1)
            images.append(state.accum[..., :3].copy())
        samples.setflags(write=False)
        _truth_cache[key] = (samples, images)
    return _truth_cache[key]


def checkpoints(every, cap, start=0):
    out, n = [], start
    while n < cap:
        n = min(n + every, cap)
        out.append(n)
    return out


def table_from_samples(samples, every, cap):
    """{spp at a check: block mean noise (float64, one per block, ascending block index)} of the UNIFORM image"""
    out = {}
    for n in checkpoints(every, cap):
        t = T.truth(samples, n)
        out[n] = t["sum"] / t["count"]
    return out


def choose_target(table, nominal):
    """The geometric mean of the two neighbouring table entries around `nominal`, and the assertion that no entry is within 4 x 2^-40 of it."""
    entries = np.sort(np.unique(np.concatenate([v[v > 0] for v in table.values()])))
    hi = int(np.searchsorted(entries, nominal))
    assert 0 < hi < len(entries), "the nominal target lies outside the table"
    target = float((entries[hi - 1] * entries[hi]) ** 0.5)
    allv = np.concatenate(list(table.values()))
    assert (np.abs(allv - target) > 4 * REL * target).all(), "a table entry is too close to the target"
    print("target %.9g between the table entries %.6f and %.6f" % (target, entries[hi - 1], entries[hi]))
    return target


def schedule(table, target, every, min_spp, cap, start=0, frozen=None):
    """spp_b per block and the final frame counter, from the semantics: after every step, from min_spp on, an active block with mean <= target freezes;
    the loop ends when none is active or at the cap.  `frozen`: {block: spp_b} of an earlier call."""
    nb = len(next(iter(table.values())))
    frozen = dict(frozen or {})
    counter = start
    for n in checkpoints(every, cap, start):
        counter = n
        if n >= min_spp:
            for b in range(nb):
                if b not in frozen and table[n][b] <= target:
                    frozen[b] = n
        if len(frozen) == nb:
            break
    return np.array([frozen.get(b, counter) for b in range(nb)], np.int32), counter, frozen


def assert_diverse(spp_b, frozen, min_spp, every, cap, full):
    """A failure, not a skip.  `full` (the 100 x 75 tiny0 case, with and without sun visibility): at least 3 distinct freeze counts, a block frozen at the
    first eligible check and one still active at the cap.  The sibenik case freezes at 16 / 24 / 32 / 40 / 48 and the 96 x 64 case at 6 / 12 / 18 / 36 / 48,
    everything by the cap (computed with the oracle): of those the distinct counts are asserted."""
    first = min(n for n in checkpoints(every, cap) if n >= min_spp)
    counts = set(frozen.values())
    print("schedule:", dict(sorted(frozen.items())), "| still active at the cap:", [b for b in range(len(spp_b)) if b not in frozen])
    assert len(counts) >= 3, "fewer than 3 distinct freeze counts"
    if full:
        assert first in counts, "no block freezes at the first eligible check"
        assert len(frozen) < len(spp_b), "no block is still active at the cap"


def block_slices(w, h):
    nbx, nby = (w + B - 1) // B, (h + B - 1) // B
    return [(slice(by * B, (by + 1) * B), slice(bx * B, (bx + 1) * B)) for by in range(nby) for bx in range(nbx)]


def per_block(w, h, spp_b, of_spp, shape_tail=(), dtype=np.float32):
    """the image whose block b is of_spp(spp_b[b])'s"""
    out = np.zeros((h, w) + shape_tail, dtype)
    made = {}
    for b, (ys, xs) in enumerate(block_slices(w, h)):
        n = int(spp_b[b])
        if n not in made:
            made[n] = of_spp(n)
        out[ys, xs] = made[n][ys, xs]
    return out


def expected(samples, images, w, h, spp_b):
    def mom(n):
        mean, m2 = T.moments(samples[:n])
        return np.stack([mean, m2], -1)

    def noise(n):
        mean, m2 = T.moments(samples[:n])
        return T.noise_e(mean, m2, n)
    e = per_block(w, h, spp_b, noise)
    idx, s, cnt = T.blocks(e)
    return dict(image=per_block(w, h, spp_b, lambda n: images[n - 1], (3,)), moments=per_block(w, h, spp_b, mom, (2,)), e=e, idx=idx, sum=s, count=cnt,
                numbers=T.image_numbers(idx, s, cnt, w * h), pixel_samples=int((cnt.astype(np.int64) * spp_b.astype(np.int64)).sum()))


def _close(a, b):
    return abs(a - b) <= REL * abs(b)


def assert_state(p, want, spp_b, counter, w, h, tag=""):
    assert p.GetSPP() == counter, tag
    idx, spp = p.ReadBlockSPP()
    assert np.array_equal(idx, want["idx"]) and np.array_equal(spp, spp_b), "%s ReadBlockSPP %s, expected %s" % (tag, spp, spp_b)
    assert np.array_equal(p.ReadSPP(), per_block(w, h, spp_b, lambda n: np.full((h, w), n, np.int32), (), np.int32)), tag
    assert np.array_equal(bits(p.ReadResult()), bits(want["image"])), "image " + tag
    assert np.array_equal(bits(p.ReadNoiseMoments()), bits(want["moments"])), "moments " + tag
    assert np.array_equal(bits(p.ReadNoise()), bits(want["e"])), "per-pixel noise " + tag
    bi, s, cnt = p.ReadBlockNoise()
    assert np.array_equal(bi, want["idx"]) and np.array_equal(cnt, want["count"]), tag
    rel = np.abs(s - want["sum"]) / np.maximum(want["sum"], np.finfo(np.float64).tiny)
    print("largest relative error of a block sum: %.3g (bound %.3g)" % (rel.max(), REL))
    assert (rel <= REL).all(), tag
    g = p.GetNoise()
    mean_noise, worst_block, worst_index, gap = want["numbers"]
    assert g["spp"] == counter and g["pixels"] == w * h
    assert _close(g["mean_noise"], mean_noise) and _close(g["worst_block"], worst_block), tag
    assert gap > 2 * REL * worst_block and g["worst_index"] == worst_index, tag
    return g


def assert_result(r, want, spp_b, counter, n_frozen):
    mean_noise, worst_block, worst_index, _ = want["numbers"]
    assert r["spp"] == counter and r["blocks"] == len(spp_b) and r["blocks_frozen"] == n_frozen and r["pixel_samples"] == want["pixel_samples"], r
    assert _close(r["mean_noise"], mean_noise) and _close(r["worst_block"], worst_block) and r["worst_index"] == worst_index and r["pixels"] == int(want["count"].sum()), r


def plan_of(case, samples):
    name, w, h, life, sub, every, min_spp, cap, nominal = case
    table = table_from_samples(samples, every, cap)
    print("block means at the checks:", {n: np.round(v, 4).tolist() for n, v in table.items()})
    target = choose_target(table, nominal)
    spp_b, counter, frozen = schedule(table, target, every, min_spp, cap)
    assert_diverse(spp_b, frozen, min_spp, every, cap, full=case is TINY0)
    return table, target, spp_b, counter, frozen


VARIANTS = [(TINY0, "fif1"), (TINY0, "fif5"), (TINY0, "fif128"), (TINY0, "launch_per_bounce"), (TINY0, "sun_visibility"), (SIBENIK, "default"), (SMALL, "default"),
            (SMALL, "fif1")]


@pytest.mark.parametrize("case,variant", VARIANTS, ids=lambda v: v if isinstance(v, str) else "%s-%dx%d-life%d-every%d" % (v[0], v[1], v[2], v[3], v[5]))
def test_adaptive_is_the_uniform_image_per_block(case, variant, scene_cache, sobol_matrices):
    name, w, h, life, sub, every, min_spp, cap, nominal = case
    inst, _ = _instance(scene_cache, case)
    p = inst.m_path_tracer
    sun = variant == "sun_visibility"
    samples, images = _truth(inst, case, sobol_matrices, sun)
    table, target, spp_b, counter, frozen = plan_of(case, samples)
    want = expected(samples, images, w, h, spp_b)
    if variant.startswith("fif"):
        p.SetFramesInFlight(int(variant[3:]))
    if variant == "launch_per_bounce":
        p.SetFusedBounces(False)
    if sun:
        p.SetSunVisibility(True)
    p.SetNoiseStats(True)
    r = p.TraceAdaptive(target, min_spp, cap, every)
    if variant == "launch_per_bounce":
        assert not p.GetFusedBounces()
    assert_result(r, want, spp_b, counter, len(frozen))
    assert_state(p, want, spp_b, counter, w, h, variant)
    p.destroy()


def test_sub_pixel_jitter_beyond_the_first_group(scene_cache, sobol_matrices):
    """tmpLifetime 2, subpixel 3: no exact CPU samples beyond the first group, so the reference is the library's own UNIFORM run, snapshots of ReadResult /
    ReadNoiseMoments / ReadNoise / ReadBlockNoise at every check (as tests/test_gpu_noise.py holds schedules against each other there); the first check
    of that run is held against the numpy truth."""
    case = ("tiny0", 72, 40, 2, 3, 4, 4, 32, 0.1)
    name, w, h, life, sub, every, min_spp, cap, nominal = case
    inst, _ = _instance(scene_cache, case)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    snap, table = {}, {}
    for n in checkpoints(every, cap):
        p.Trace(True, n - p.GetSPP())
        idx, s, cnt = p.ReadBlockNoise()
        snap[n] = (p.ReadResult(), p.ReadNoiseMoments(), p.ReadNoise(), s)
        table[n] = s / cnt
    p.Reset()
    target = choose_target(table, nominal)
    spp_b, counter, frozen = schedule(table, target, every, min_spp, cap)
    print("schedule:", spp_b.tolist(), "counter", counter)
    assert len(set(frozen.values())) >= 2 and 0 < len(frozen)
    r = p.TraceAdaptive(target, min_spp, cap, every)
    assert p.GetSPP() == counter and r["spp"] == counter and r["blocks_frozen"] == len(frozen)
    assert np.array_equal(p.ReadBlockSPP()[1], spp_b)
    got = (p.ReadResult(), p.ReadNoiseMoments(), p.ReadNoise(), p.ReadBlockNoise()[1])
    for k, tail in enumerate([(3,), (2,), ()]):
        assert np.array_equal(bits(got[k]), bits(per_block(w, h, spp_b, lambda n: snap[n][k], tail))), "read-out %d" % k
    assert np.array_equal(got[3].view(np.uint64), np.array([snap[int(n)][3][b] for b, n in enumerate(spp_b)]).view(np.uint64))
    assert r["pixel_samples"] == int((cnt.astype(np.int64) * spp_b).sum())
    p.destroy()


def test_zero_variance_freezes_everything_at_the_first_eligible_check(scene_cache):
    spec = scenes.make_scene("tiny2", scene_cache, width=64, height=48, pt={"tmpLifetime": 4, "maxBounce": 4, "subpixel": 1})
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=SEED), api.InstanceConfig.last_error()
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    r = p.TraceAdaptive(0.0, 6, 40, 3)
    assert p.GetSPP() == 6 and r["spp"] == 6 and r["blocks"] == 4 and r["blocks_frozen"] == 4 and r["pixel_samples"] == 6 * 64 * 48
    assert r["mean_noise"] == 0.0 and r["worst_block"] == 0.0 and not p.ReadNoise().any()
    assert np.array_equal(p.ReadBlockSPP()[1], np.full(4, 6, np.int32))
    img = p.ReadResult()
    p.Trace(True, 5)  # every block frozen: the counter advances, no kernel runs, nothing changes
    assert p.GetSPP() == 11 and np.array_equal(bits(p.ReadResult()), bits(img)) and np.array_equal(p.ReadBlockSPP()[1], np.full(4, 6, np.int32))
    p.Reset()
    p.Trace(True, 6)
    assert np.array_equal(bits(p.ReadResult()), bits(img))  # (zero variance: the uniform 6 spp image)
    p.destroy()


def test_state_rules(scene_cache, sobol_matrices):
    case = TINY0
    name, w, h, life, sub, every, min_spp, cap, nominal = case
    inst, _ = _instance(scene_cache, case)
    p = inst.m_path_tracer
    samples, images = _truth(inst, case, sobol_matrices)
    table, target, spp_b, counter, frozen = plan_of(case, samples)
    # works with the statistics off: every block at the counter
    assert np.array_equal(p.ReadBlockSPP()[1], np.zeros(12, np.int32))
    p.Trace(True, 3)
    before = p.ReadResult()

    def refused(code, *args):
        with pytest.raises(N.AdyptError) as e:
            p.TraceAdaptive(*args)
        assert e.value.code == code and p.GetSPP() == 3 and np.array_equal(bits(p.ReadResult()), bits(before)), args
    refused(N.E_STATE, target, min_spp, cap, every)  # the statistics are off
    p.Reset()
    p.SetNoiseStats(True)
    p.Trace(True, 3)
    for bad in ((target, 8, 64, 0), (target, 1, 64, 8), (target, 16, 8, 8), (target, 0, 0, 8), (float("nan"), 8, 64, 8)):
        refused(N.E_INVALID, *bad)
    p.SetLookahead(True)
    refused(N.E_STATE, target, min_spp, cap, every)  # look-ahead enabled
    p.SetFramesInFlight(5)
    p.Reset()
    p.Trace(True, 3)  # parks frames 3, 4 ahead
    assert p.GetLookaheadFrames() == 2
    refused(N.E_STATE, target, min_spp, cap, every)
    p.SetLookahead(False)
    p.Reset()
    # an adaptive run to the middle of the schedule: cap 32
    spp32, counter32, frozen32 = schedule(table, target, every, min_spp, 32)
    r = p.TraceAdaptive(target, min_spp, 32, every)
    want = expected(samples, images, w, h, spp32)
    assert_result(r, want, spp32, counter32, len(frozen32))
    assert_state(p, want, spp32, counter32, w, h, "cap 32")
    assert 0 < len(frozen32) < 12
    with pytest.raises(N.AdyptError) as e:
        p.SetNoiseStats(False)  # blocks are frozen: reset first
    assert e.value.code == N.E_STATE and p.GetNoiseStats()
    # Trace(True, n) changes no bit of a frozen block and advances the active ones to the uniform image; SetCamera keeps the set
    ip, iv = inst.m_camera.matrices()
    p.SetCamera(ip, iv, inst.m_camera.position)
    p.Trace(True, 5)
    spp37 = np.array([frozen32.get(b, 37) for b in range(12)], np.int32)
    assert_state(p, expected(samples, images, w, h, spp37), spp37, 37, w, h, "Trace(True, 5) after the adaptive run")
    # TraceUntil traces the active blocks only, too
    p.TraceUntil(0.0, 2, 40, 3)
    spp40 = np.array([frozen32.get(b, 40) for b in range(12)], np.int32)
    assert_state(p, expected(samples, images, w, h, spp40), spp40, 40, w, h, "TraceUntil after the adaptive run")
    # a second adaptive call with a lower target leaves the frozen blocks alone: the table decides about the others from 40 spp on
    table2 = {n: v for n, v in table.items() if n > 40}
    target2 = choose_target(table2, 0.09)
    spp_2, counter_2, frozen_2 = schedule(table, target2, every, min_spp, cap, start=40, frozen=frozen32)
    assert all(frozen_2[b] == n for b, n in frozen32.items()) and counter_2 > 40
    r = p.TraceAdaptive(target2, min_spp, cap, every)
    want = expected(samples, images, w, h, spp_2)
    assert_result(r, want, spp_2, counter_2, len(frozen_2))
    assert_state(p, want, spp_2, counter_2, w, h, "second adaptive call")
    # Reset() thaws: the uniform 5 spp image everywhere
    p.Reset()
    p.Trace(True, 5)
    five = np.full(12, 5, np.int32)
    assert_state(p, expected(samples, images, w, h, five), five, 5, w, h, "after Reset")
    # Trace(False) thaws
    p.TraceAdaptive(target, min_spp, 16, every)
    assert (p.ReadBlockSPP()[1] != 16).any()
    p.Trace(False)
    assert p.GetSPP() == 0 and not p.ReadBlockSPP()[1].any()
    p.Trace(True, 7)
    seven = np.full(12, 7, np.int32)
    assert_state(p, expected(samples, images, w, h, seven), seven, 7, w, h, "after a viewer frame")
    p.SetNoiseStats(False)  # nothing frozen: allowed again
    p.destroy()


# nominal targets from the oracle's tables of these two shapes (check every 4 to 24 spp): 100 x 75 freezes at 4 / 8 / 12 / 16 / 20 with block 5 still active at
# the cap, 64 x 36 (two of its four blocks without noise) at 4 / 16 / 20
@pytest.mark.parametrize("shape,n_dev,nominal", [((100, 75), 3, 0.16), ((64, 36), 4, 0.1)], ids=["100x75-3-shards", "64x36-4-shards-one-owns-nothing"])
def test_multi_device_on_one_card(shape, n_dev, nominal, scene_cache, monkeypatch):
    """Several shards on one card against one device: identical, whatever the numbers are (the one-device numbers are held against the truth above)."""
    monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
    w, h = shape
    case = ("tiny0", w, h, 4, 1)
    inst, _ = _instance(scene_cache, case)
    single = inst.m_path_tracer
    c = inst.m_config
    m = api.MultiPathTracer()
    m.Initialize(c.pt_params(SEED), inst.m_hipscene, c.m_width, c.m_height, (0,) * n_dev)
    ip, iv = inst.m_camera.matrices()
    m.SetCamera(ip, iv, inst.m_camera.position)
    assert m.DeviceCount() == n_dev
    single.SetNoiseStats(True)
    m.SetNoiseStats(True)
    # the target from a uniform run of the single device: between two block means of its table, so that blocks freeze at different checks
    every, min_spp, cap = 4, 4, 24
    table = {}
    for n in checkpoints(every, cap):
        single.Trace(True, every)
        idx, s, cnt = single.ReadBlockNoise()
        table[n] = s / cnt
    single.Reset()
    target = choose_target(table, nominal)
    spp_b, counter, frozen = schedule(table, target, every, min_spp, cap)
    print("schedule:", spp_b.tolist())
    assert len(set(frozen.values())) >= 3 and min_spp in frozen.values(), "the schedule does not freeze at three checks, the first eligible one among them"
    if n_dev == 3:
        assert len(frozen) < len(spp_b), "no block is still active at the cap"
    rs, rm = single.TraceAdaptive(target, min_spp, cap, every), m.TraceAdaptive(target, min_spp, cap, every)
    assert rm == rs and rs["blocks"] == len(spp_b) and rs["blocks_frozen"] == len(frozen) and rs["pixels"] == w * h
    assert single.GetSPP() == counter and m.GetSPP() == counter
    a, b = m.ReadBlockSPP(), single.ReadBlockSPP()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(b[1], spp_b)
    assert np.array_equal(m.ReadSPP(), single.ReadSPP())
    assert np.array_equal(bits(m.ReadResult()), bits(single.ReadResult()))  # (through the gather)
    assert np.array_equal(bits(m.ReadNoiseMoments()), bits(single.ReadNoiseMoments()))
    assert np.array_equal(bits(m.ReadNoise()), bits(single.ReadNoise()))
    assert m.GetNoise() == single.GetNoise()
    a, b = m.ReadBlockNoise(), single.ReadBlockNoise()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and np.array_equal(a[2], b[2])
    # tracing on: the active blocks only, on every device
    single.Trace(True, 3)
    m.Trace(True, 3)
    assert np.array_equal(bits(m.ReadResult()), bits(single.ReadResult())) and np.array_equal(m.ReadBlockSPP()[1], single.ReadBlockSPP()[1])
    m.destroy()
    single.destroy()


def test_cli_adaptive(scene_cache, sobol_matrices, tmp_path):
    case = TINY0
    name, w, h, life, sub, every, min_spp, cap, nominal = case
    inst, spec = _instance(scene_cache, case)
    samples, images = _truth(inst, case, sobol_matrices)
    table, target, spp_b, counter, frozen = plan_of(case, samples)
    p = inst.m_path_tracer
    p.SetNoiseStats(True)
    g = p.TraceAdaptive(target, min_spp, cap, every)
    img, e, spp_map = p.ReadResult(), p.ReadNoise(), p.ReadSPP()
    p.destroy()
    assert np.array_equal(bits(img), bits(expected(samples, images, w, h, spp_b)["image"]))
    a_exr, n_exr, s_exr = str(tmp_path / "a.exr"), str(tmp_path / "n.exr"), str(tmp_path / "s.exr")
    r = subprocess.run([CLI, spec.config_path, "--noise", repr(target), "--adaptive", "--spp", str(cap), "--check-every", str(every), "--min-spp", str(min_spp), "--out", a_exr,
                        "--noise-out", n_exr, "--spp-out", s_exr, "--seed", str(SEED)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    text = (r.stdout + r.stderr).decode()
    assert r.returncode == 0, text[-2000:]
    line = re.search(r"\[PT\]ADAPTIVE: spp (\d+) frozen (\d+) of (\d+) pixel_samples (\d+) \(uniform (\d+)\) mean_noise (\S+) worst_block (\S+) worst_index (-?\d+)", text)
    assert line, text[-2000:]
    assert [int(line.group(k)) for k in (1, 2, 3, 4, 5, 8)] == [g["spp"], g["blocks_frozen"], g["blocks"], g["pixel_samples"], g["spp"] * w * h, g["worst_index"]]
    assert float(line.group(6)) == float("%.9g" % g["mean_noise"]) and float(line.group(7)) == float("%.9g" % g["worst_block"])
    assert "[PT]NOISE" not in text
    assert np.array_equal(bits(api.load_exr(a_exr)), bits(img))
    grey, count = api.load_exr(n_exr), api.load_exr(s_exr)
    for ch in range(3):
        assert np.array_equal(bits(grey[..., ch]), bits(e))
        assert np.array_equal(count[..., ch], spp_map.astype(np.float32))
    # without --adaptive the CLI is what it was: the uniform render to the noise target
    wb = {n: float(v.max()) for n, v in table.items()}
    stop = min(n for n in checkpoints(every, cap) if n >= min_spp and (wb[n] <= target or n == cap))
    r = subprocess.run([CLI, spec.config_path, "--noise", repr(target), "--spp", str(cap), "--check-every", str(every), "--min-spp", str(min_spp), "--out", a_exr, "--seed", str(SEED)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    text = (r.stdout + r.stderr).decode()
    assert r.returncode == 0 and "ADAPTIVE" not in text and re.search(r"\[PT\]NOISE: spp %d " % stop, text), text[-2000:]
    assert np.array_equal(bits(api.load_exr(a_exr)), bits(images[stop - 1]))
