"""The noise estimate's definition (csrc/device/noise.hpp) compiled on the host and held bit for bit against its numpy float32 restatement
(tests/noise_truth.py), on exact per-frame samples from the CPU oracle and on hand-made edge values.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import noise_truth as T
from tests.helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE = os.path.join(ROOT, "adypt_amd", "csrc", "device")

DRIVER = r"""
#include "noise.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace adypt;
// moments IN OUT: int32 n_px, n_frames, first; float32 samples[n_frames][n_px][3]  ->  float32 (mean, m2)[n_px] after every frame, then e[n_px] after the last
// image IN OUT:   int64 n, pixels; int32 index[n]; double sum[n]; uint32 count[n]  ->  double mean_noise, worst_block; int32 worst_index
int main(int argc, char **argv)
{
	if(argc != 4) return 2;
	FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
	if(!in || !out) return 3;
	if(argv[1][0] == 'm')
	{
		int32_t h[3];
		if(fread(h, 4, 3, in) != 3) return 4;
		const size_t n_px = (size_t)h[0];
		std::vector<float> s(n_px * 3);
		std::vector<NoiseMoments> m(n_px, NoiseMoments{0.0f, 0.0f});
		for(int k = 0; k < h[1]; ++k)
		{
			if(fread(s.data(), 4, s.size(), in) != s.size()) return 4;
			for(size_t i = 0; i < n_px; ++i) m[i] = noise_add_sample(m[i], h[2] + k, s[3 * i], s[3 * i + 1], s[3 * i + 2]);
			fwrite(m.data(), sizeof(NoiseMoments), n_px, out);
		}
		std::vector<float> e(n_px);
		for(size_t i = 0; i < n_px; ++i) e[i] = noise_of_pixel(m[i], h[2] + h[1]);
		fwrite(e.data(), 4, n_px, out);
	}
	else
	{
		int64_t h[2];
		if(fread(h, 8, 2, in) != 2) return 4;
		const size_t n = (size_t)h[0];
		std::vector<int32_t> index(n); std::vector<double> sum(n); std::vector<uint32_t> count(n);
		if(fread(index.data(), 4, n, in) != n || fread(sum.data(), 8, n, in) != n || fread(count.data(), 4, n, in) != n) return 4;
		std::vector<BlockState> blocks(n);
		for(size_t i = 0; i < n; ++i) blocks[i] = BlockState{index[i], sum[i], count[i], 0, false};
		const NoiseImage r = noise_of_image(blocks.data(), n, h[1]);
		fwrite(&r.mean_noise, 8, 1, out); fwrite(&r.worst_block, 8, 1, out); fwrite(&r.worst_index, 4, 1, out);
	}
	fclose(out);
	return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("noise_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", DEVICE, src, "-o", exe])
    return exe, str(d)


def run_moments(driver, samples, first=0):
    """samples (n_frames, ..., 3) -> (mean, m2) after every frame (n_frames, ...) and e after the last (...)."""
    exe, d = driver
    shape = samples.shape[1:-1]
    flat = np.ascontiguousarray(samples, dtype=np.float32).reshape(samples.shape[0], -1, 3)
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(np.array([flat.shape[1], flat.shape[0], first], np.int32).tobytes())
        f.write(flat.tobytes())
    subprocess.check_call([exe, "m", os.path.join(d, "in.bin"), os.path.join(d, "out.bin")])
    raw = np.fromfile(os.path.join(d, "out.bin"), dtype=np.float32)
    n_px, n = flat.shape[1], flat.shape[0]
    mom = raw[:n * n_px * 2].reshape((n,) + shape + (2,))
    return mom[..., 0], mom[..., 1], raw[n * n_px * 2:].reshape(shape)


def run_image(driver, idx, s, cnt, pixels):
    exe, d = driver
    with open(os.path.join(d, "img.bin"), "wb") as f:
        f.write(np.array([len(idx), pixels], np.int64).tobytes())
        f.write(np.asarray(idx, np.int32).tobytes() + np.asarray(s, np.float64).tobytes() + np.asarray(cnt, np.uint32).tobytes())
    subprocess.check_call([exe, "i", os.path.join(d, "img.bin"), os.path.join(d, "img_out.bin")])
    raw = open(os.path.join(d, "img_out.bin"), "rb").read()
    return float(np.frombuffer(raw, np.float64, 2)[0]), float(np.frombuffer(raw, np.float64, 2)[1]), int(np.frombuffer(raw, np.int32, 1, 16)[0])


def test_header_needs_no_hip_include_and_has_no_fma():
    text = open(os.path.join(DEVICE, "noise.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "hip" not in "".join(l for l in code.splitlines() if l.startswith("#include")).lower()
    assert "fma" not in code
    # g++ alone compiles it (no HIP on the include path), warnings as errors
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", DEVICE, "-x", "c++", "-"],
                   input=b'#include "noise.hpp"\nint main() { return (int)adypt::noise_of_pixel(adypt::NoiseMoments{1.0f, 1.0f}, 2); }\n', check=True)


def check_against_numpy(driver, samples):
    mean, m2, e = run_moments(driver, samples)
    n = samples.shape[0]
    tm, t2 = None, None
    for k in range(n):  # after every frame
        tm, t2 = T.moments(samples[k:k + 1], tm, t2, first=k)
        assert np.array_equal(bits(mean[k]), bits(tm)) and np.array_equal(bits(m2[k]), bits(t2)), "moments after frame %d" % k
    te = T.noise_e(tm, t2, n)
    assert np.array_equal(bits(e), bits(te))
    assert np.isfinite(e).all() and (e >= 0).all() and (m2 >= 0).all()
    return tm, t2, te


@pytest.mark.parametrize("w,h,life,sub,spp", [(100, 75, 16, 3, 16), (96, 64, 4, 1, 64)])
def test_definition_on_exact_oracle_samples(w, h, life, sub, spp, driver, scene_cache, sobol_matrices):
    """The two configurations whose CPU samples are exact (k < tmpLifetime, or subpixel == 1): first that they ARE — folded through the running mean
    they give the oracle's own image, every word — then the header against numpy on them, after every frame; then the image numbers."""
    from adypt_amd import api, scenes
    spec = scenes.make_scene("tiny0", scene_cache, width=w, height=h, pt={"tmpLifetime": life, "maxBounce": 6, "subpixel": sub})
    cfg = api.InstanceConfig()
    assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
    sc = api.Scene()
    assert sc.LoadFromFile(cfg.m_obj_filename)
    b = api.WideBVH()
    if not b.LoadFromFile(cfg.m_bvh_filename, cfg.bvh_params()):
        b.Build(sc, cfg.bvh_params())
        assert b.SaveToFile(cfg.m_bvh_filename, cfg.bvh_params())
    osc = O.Scene(b.nodes, b.tri_indices, sc.triangles, sc.materials, textures=sc.textures)
    P, shift = T.oracle_params(cfg.c), O.shift_bytes(31, w, h)
    samples = T.frame_samples(osc, P, shift, sobol_matrices, spp)
    state = O.PathTracerState(w, h)
    O.pt_frames(osc, P, shift, sobol_matrices, state, spp)
    differing = int((bits(T.running_mean(samples)) != bits(state.accum[..., :3])).sum())
    assert differing == 0, "%d words of the folded samples differ from the oracle's image" % differing
    assert (samples <= np.float32(cfg.c.clamp)).all() and (samples == np.float32(cfg.c.clamp)).any()  # values AT the clamp are among them
    _, _, e = check_against_numpy(driver, samples)
    idx, s, cnt = T.blocks(e)
    assert int(cnt.sum()) == w * h
    mean_noise, worst_block, worst_index, gap = T.image_numbers(idx, s, cnt, w * h)
    got = run_image(driver, idx, s, cnt, w * h)
    assert got == (mean_noise, worst_block, worst_index)
    assert 0.0 < mean_noise < worst_block and gap > 0.0


def test_definition_on_edge_values(driver):
    c = np.float32(4.0)
    n = 12
    px = {
        "all zero": np.zeros((n, 3), np.float32),
        "constant": np.tile(np.array([0.25, 0.5, 0.75], np.float32), (n, 1)),
        "constant at the clamp": np.full((n, 3), c, np.float32),
        "one bright sample among zeros": np.concatenate([np.zeros((5, 3), np.float32), np.full((1, 3), c, np.float32), np.zeros((n - 6, 3), np.float32)]),
        "first sample bright": np.concatenate([np.full((1, 3), c, np.float32), np.zeros((n - 1, 3), np.float32)]),
        "alternating 0 / clamp": np.array([[0, 0, 0], [c, c, c]] * (n // 2), np.float32),
        "tiny": np.full((n, 3), np.float32(1e-30), np.float32) * np.arange(1, n + 1, dtype=np.float32)[:, None],
    }
    names = list(px)
    samples = np.stack([px[k] for k in names], axis=1)  # (n, pixels, 3)
    mean, m2, e = check_against_numpy(driver, samples)
    r = dict(zip(names, zip(mean, m2, e)))
    assert r["all zero"] == (0.0, 0.0, 0.0)
    assert r["constant"][1] == 0.0 and r["constant"][2] == 0.0 and r["constant at the clamp"][1] == 0.0
    assert r["one bright sample among zeros"][1] > 0.0 and r["one bright sample among zeros"][2] > 0.5
    # two frames are the fewest the estimate is defined for
    check_against_numpy(driver, samples[:2])


def test_image_numbers_ties_and_empty_blocks(driver):
    # a tie takes the lowest index; blocks of no pixels (a shard's view of blocks it does not own) count for nothing
    idx = np.array([0, 1, 2, 3, 4], np.int32)
    s = np.array([10.0, 30.0, 0.0, 30.0, 3.0], np.float64)
    cnt = np.array([10, 20, 0, 20, 4], np.uint32)
    mean_noise, worst_block, worst_index = run_image(driver, idx, s, cnt, 54)
    assert (mean_noise, worst_block, worst_index) == (((10.0 + 30.0) + 30.0 + 3.0) / 54.0, 1.5, 1)
    assert run_image(driver, idx[:0], s[:0], cnt[:0], 0) == (0.0, 0.0, 0)
    # an all-zero image is a result, not "nothing covered"
    assert run_image(driver, idx, np.zeros(5), cnt, 54) == (0.0, 0.0, 0)


def test_plan_parks_the_lone_frame_when_statistics_are_on(tmp_path):
    """frame_plan.hpp: PlanInput::noise_stats defaults to 0 and changes nothing at 0; at 1 the lone launch-per-bounce frame becomes a batch of one that
    keeps its launches (no k_path) and parks its sample for the running-mean kernel."""
    src = tmp_path / "plan.cpp"
    src.write_text(r'''
#include "frame_plan.hpp"
#include <cstdio>
using namespace adypt;
int main()
{
	int bad = 0, lone = 0;
	for(int spp : {0, 1, 5}) for(int remaining : {1, 3}) for(int la : {0, 1}) for(int fif : {1, 4}) for(int life : {1, 4}) for(int sf : {0, 1}) for(int ff : {0, 1}) for(int fb : {0, 1}) for(int sun : {0, 1})
	{
		PlanInput in;
		in.spp = spp; in.remaining = remaining; in.lookahead = la; in.frames_in_flight = fif; in.tmp_lifetime = life; in.max_bounce = 5; in.pipeline = 1;
		in.single_fused = sf; in.first_fused = ff; in.fused_bounces = fb; in.sun_visibility = sun; in.n_local_px = 6144;
		if(in.noise_stats != 0) ++bad;
		const PassPlan off = plan_pass(in);
		in.noise_stats = 1;
		const PassPlan on = plan_pass(in);
		if(!on.as_batch || !on.use_cache) ++bad;                    // every sample is parked
		if(on.kind != off.kind || on.m != off.m || on.hand_out != off.hand_out || on.n_pipes != off.n_pipes) ++bad;
		if(off.as_batch) { if(on.fused_bounces != off.fused_bounces || on.fused_first != off.fused_first || on.sun_query != off.sun_query || on.sun_queue != off.sun_queue) ++bad; }
		else { ++lone; if(on.fused_bounces || on.sun_query || (sun && !on.sun_queue)) ++bad; }
	}
	printf("%d %d\n", bad, lone);
	return 0;
}
''')
    exe = str(tmp_path / "plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", DEVICE, str(src), "-o", exe])
    bad, lone = (int(v) for v in subprocess.check_output([exe]).split())
    assert bad == 0 and lone > 0


UNTIL_DRIVER = r"""
#include "trace_until.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
// argv: target min_spp max_spp check_every start_spp worst_block...   (the scripted answers of the noise reads, in order; the last one repeats)
// OUT: code | out.spp out.worst_block out.mean_noise | the steps traced | the spp at which the noise was read | the message
int main(int argc, char **argv)
{
	if(argc < 7) return 2;
	const double target = atof(argv[1]);
	const int min_spp = atoi(argv[2]), max_spp = atoi(argv[3]), check_every = atoi(argv[4]);
	int spp = atoi(argv[5]);
	std::vector<double> script;
	for(int i = 6; i < argc; ++i) script.push_back(atof(argv[i]));
	std::vector<int> steps, reads;
	adypt_noise out;
	out.spp = -7; out.worst_block = -7.0; out.mean_noise = -7.0; out.worst_index = -7; out.pixels = -7; // (untouched when the call is refused)
	std::string error;
	const int r = adypt::trace_until("driver", &error, target, min_spp, max_spp, check_every, &out, [&] { return spp; },
	                                 [&](int n) { steps.push_back(n); spp += n; return ADYPT_OK; },
	                                 [&](adypt_noise *o) { o->worst_block = script[reads.size() < script.size() ? reads.size() : script.size() - 1]; o->mean_noise = 0.5 * o->worst_block; reads.push_back(spp); return ADYPT_OK; });
	printf("%d | %d %.17g %.17g |", r, out.spp, out.worst_block, out.mean_noise);
	for(int n : steps) printf(" %d", n);
	printf(" |");
	for(int n : reads) printf(" %d", n);
	printf(" | %s\n", error.c_str());
	return 0;
}
"""


@pytest.fixture(scope="module")
def until(tmp_path_factory):
    d = tmp_path_factory.mktemp("until_driver")
    src, exe = str(d / "driver.cpp"), str(d / "driver")
    open(src, "w").write(UNTIL_DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", DEVICE, src, "-o", exe])  # (the loop needs neither hipcc nor a HIP include)

    def run(target, min_spp, max_spp, check_every, start_spp, script):
        line = subprocess.check_output([exe] + [repr(v) for v in (target, min_spp, max_spp, check_every, start_spp)] + [repr(float(v)) for v in script]).decode()
        code, out, steps, reads, message = (f.strip() for f in line.split("|"))
        spp, worst, mean = out.split()
        return {"code": int(code), "spp": int(spp), "worst_block": float(worst), "mean_noise": float(mean), "steps": [int(v) for v in steps.split()],
                "reads": [int(v) for v in reads.split()], "message": message}
    return run


def test_trace_until_loop_on_scripted_noise(until):
    """The loop both adypt_trace_until and adypt_multi_trace_until run (csrc/device/trace_until.hpp), stepped over scripted noise values."""
    # target met at the first check with spp >= min_spp: it stops there
    r = until(0.1, 16, 1024, 16, 0, [0.05])
    assert (r["code"], r["steps"], r["reads"], r["spp"], r["worst_block"], r["mean_noise"]) == (0, [16], [16], 16, 0.05, 0.025)
    r = until(0.1, 2, 1024, 4, 0, [0.1])  # (at the target is met)
    assert (r["code"], r["steps"], r["reads"], r["spp"]) == (0, [4], [4], 4)
    # target met below min_spp: it goes on, and stops at the first check from min_spp on
    r = until(0.1, 16, 1024, 4, 0, [0.05])
    assert (r["code"], r["steps"], r["reads"], r["spp"]) == (0, [4, 4, 4, 4], [4, 8, 12, 16], 16)
    r = until(0.1, 10, 1024, 4, 0, [0.05])
    assert (r["steps"], r["spp"]) == ([4, 4, 4], 12)
    # met only later: every step is followed by one read, the answer of the last read is returned
    r = until(0.1, 2, 1024, 8, 0, [0.9, 0.5, 0.2, 0.09])
    assert (r["code"], r["steps"], r["reads"], r["spp"], r["worst_block"]) == (0, [8, 8, 8, 8], [8, 16, 24, 32], 32, 0.09)
    # cap reached with the target unmet: stops at max_spp, the last step shortened to max_spp - spp
    r = until(0.1, 16, 40, 16, 0, [0.9])
    assert (r["code"], r["steps"], r["reads"], r["spp"], r["worst_block"]) == (0, [16, 16, 8], [16, 32, 40], 40, 0.9)
    r = until(0.1, 16, 40, 16, 35, [0.9])  # (taken up in the middle, as the CLI's --save-every does)
    assert (r["steps"], r["reads"], r["spp"]) == ([5], [40], 40)
    # a step of one frame from 0 spp: the noise is not asked below 2 spp
    r = until(0.1, 2, 3, 1, 0, [0.9])
    assert (r["steps"], r["reads"], r["spp"]) == ([1, 1, 1], [2, 3], 3)
    # called with spp >= max_spp: traces nothing and returns the current noise (none if spp < 2)
    r = until(0.1, 16, 32, 16, 32, [0.7])
    assert (r["code"], r["steps"], r["reads"], r["spp"], r["worst_block"]) == (0, [], [32], 32, 0.7)
    r = until(0.1, 16, 32, 16, 50, [0.7])
    assert (r["code"], r["steps"], r["reads"], r["spp"], r["worst_block"]) == (0, [], [50], 50, 0.7)
    # invalid arguments are rejected before anything is traced, the caller named in the message and the result untouched
    for args in [(0.1, 16, 32, 0), (0.1, 1, 32, 16), (0.1, 16, 15, 16), (float("nan"), 16, 32, 16)]:
        r = until(*args, 0, [0.05])
        assert (r["code"], r["steps"], r["reads"], r["spp"], r["worst_block"]) == (-1, [], [], -7, -7.0), args
        assert r["message"] == "driver: needs check_every >= 1, 2 <= min_spp <= max_spp and a target that is a number"
    assert until(0.1, 2, 2, 1, 0, [0.05])["message"] == ""  # (the least that is valid)
