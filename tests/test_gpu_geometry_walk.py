"""-m gpu: the walks of tests/geometry_walk.py on a context.  After every geometry call the device is held against the model in bytes (records, nodes,
reference order, Woop data, reference boxes, sizes, answers, cost, bindings); the step's 4096 rays against the CPU oracle over the arrays read back
from the device, bit for bit, and against the binary64 brute force over the MODEL's triangles (tests/helpers.check_against_fp64_truth, which shares
no header with the device); the image of four frames against the oracle, bit for bit.  A refused call must answer its code and change nothing; a
disturbance must leave the picture the oracle's for the frames traced so far.  A failure names the walk, the step and the list of operations up to
it in the form geometry_walk.replay() takes; the test at the end of this file runs such lists."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, _native as N  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from tests import geometry_walk as W  # noqa: E402
from tests import tri_record_truth as R  # noqa: E402
from tests.helpers import bits, check_against_fp64_truth  # noqa: E402
from tests.test_gpu_refit import PT, SEED, SPP, same_woop, tracer  # noqa: E402
from tests.test_refit_definition import same_bytes  # noqa: E402

EXCUSED = 4  # of 4096 rays, as tests/test_geometry_walk.py
VARIANTS = ("launch_per_bounce", "remap", "shade_bin", "two_shards")
VARIANT_SEEDS = (1, 4)
B = 32


class Walker:
    """one context on its way through a list of operations, and the oracle's picture of the frames traced since the last reset"""

    def __init__(self, case, variant, sobol_matrices, monkeypatch):
        self.multi = variant == "two_shards"
        self.w, self.h = (64, 36) if self.multi else (32, 18)  # (two shards: 2 x 2 blocks, both own some)
        if variant == "remap":
            monkeypatch.setenv("ADYPT_REF_TRIANGLES_MAX_MB", "0")  # no per-reference records: k_path remaps through the index array
        if variant == "shade_bin":
            monkeypatch.setenv("ADYPT_SHADE_BIN", "1")  # the context keeps a class byte per triangle
        if self.multi:
            monkeypatch.setenv("ADYPT_MULTI_SHARED_DEVICE", "1")
            self.p = tracer(case, case.scene, case.bvh(), self.w, self.h, cls=api.MultiPathTracer, devices=(0, 0))
            assert self.p.DeviceCount() == 2 and all(N.lib.adypt_local_pixel_count(c) > 0 for c in self.p._contexts())
        else:
            self.p = tracer(case, case.scene, case.bvh())
        if variant in ("launch_per_bounce", "shade_bin"):
            self.p.SetFusedBounces(False)
        self.fused = variant not in ("launch_per_bounce", "shade_bin")
        self.case, self.sobol = case, sobol_matrices
        self.ip, self.iv = (case.ip, case.iv) if not self.multi else api.camera_matrices(60.0, 30.0, -10.0, self.w, self.h)
        self.lookahead = False
        self.excused = 0
        self.scene_of(None)

    # -- the oracle's side --
    def scene_of(self, arrays):
        """the oracle's scene from now on: (nodes, reference order) as read back and the model's triangles; no frame traced"""
        self.arrays = arrays
        self.fresh()

    def fresh(self):
        self.state, self.frames = O.PathTracerState(self.w, self.h), 0

    def picture(self, more=0):
        """the oracle's image after `more` further frames"""
        nodes, idx, tris = self.arrays
        if more:
            c = api.InstanceConfig().c
            prm = O.make_params(self.w, self.h, list(self.case.pos), self.ip, self.iv, stack_size=PT["stack_size"], max_bounce=PT["max_bounce"], subpixel=PT["subpixel"],
                                tmp_life=PT["tmp_life"], tmin=c.ray_tmin, clamp=c.clamp, sun=list(c.sun), sun_visibility=False)
            osc = O.Scene(nodes, idx, tris, self.case.scene.materials, textures=self.case.scene.textures)
            O.pt_frames(osc, prm, O.shift_bytes(SEED, self.w, self.h), self.sobol, self.state, more)
            self.frames += more
        return self.state.accum[..., :3].copy()

    # -- the device's side --
    def trace(self, k):
        if self.lookahead:  # one frame per call, as Instance::Update asks
            for _ in range(k):
                self.p.Trace(True, 1)
        else:
            self.p.Trace(True, k)

    def read_tree(self):
        """[(nodes, Woop data, reference order)] of every context"""
        out = []
        n_nodes, n_refs = self.p.GetBVHSizes()
        for c in self.p._contexts():
            nodes, woop, idx = np.zeros(n_nodes * 80, np.uint8), np.zeros((n_refs, 12), np.float32), np.zeros(max(n_refs, 1), np.int32)
            N.check(N.lib.adypt_read_bvh(c, nodes.ctypes.data, woop.ctypes.data), c)
            N.check(N.lib.adypt_read_tri_indices(c, idx.ctypes.data), c)
            out.append((nodes, woop, idx[:n_refs]))
        return out

    def bindings(self):
        return self.p.GetPoseBinding(), self.p.GetMorphBinding(), self.p.GetMeshBinding()

    def holds(self, s):
        """records, tree and bindings are the model's"""
        p = self.p
        assert p.GetTriangleCount() == len(s.tris)
        assert p.ReadTriangles().tobytes() == s.tris.tobytes(), "ReadTriangles"
        assert p.ReadTriangleRecords().tobytes() == R.pack(s.tris, self.case.scene.materials, 0)[0].tobytes(), "ReadTriangleRecords"
        assert p.GetBVHSizes() == (len(s.nodes) // 80, len(s.tri_indices)), "GetBVHSizes"
        trees = self.read_tree()
        for k, (nodes, woop, idx) in enumerate(trees):
            assert same_bytes(nodes, s.nodes), "nodes of context %d" % k
            assert np.array_equal(idx, s.tri_indices), "reference order of context %d" % k
            assert same_woop(woop, s.woop), "Woop data of context %d" % k
        boxes = p.ReadRefBoxes()
        assert (boxes is None) == (s.ref_boxes is None), "ReadRefBoxes is %s" % (None if boxes is None else "there")
        assert boxes is None or np.array_equal(bits(boxes), bits(s.ref_boxes)), "reference boxes"
        pose, morph, mesh = self.bindings()
        for got, want, what in ((pose, s.pose, "GetPoseBinding"), (morph, s.morph, "GetMorphBinding"), (mesh, s.mesh, "GetMeshBinding")):
            assert {k: got[k] for k in want} == want and (got["device_bytes"] > 0) == any(want.values()), "%s: %s" % (what, got)
        return trees[0]

    def rays(self, s, tree):
        if self.multi:  # (a ray batch is a context's call)
            return
        nodes, woop, idx = tree
        osc = O.Scene(nodes, idx, self.p.ReadTriangles(), self.case.scene.materials, woop=woop)
        rays = s.rays()
        for any_hit in (False, True):
            want = O.trace(osc, rays, stack_size=PT["stack_size"], any_hit=any_hit)
            got = self.p.TraceRays(rays, with_stats=True, any_hit=any_hit)
            for f in api.HIT_DT.names:
                assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), "TraceRays with statistics, any_hit %s: %s" % (any_hit, f)
            bare = self.p.TraceRays(rays, with_stats=False, any_hit=any_hit)
            for f in ("tri_id", "u", "v", "t"):
                assert np.array_equal(bare[f].view(np.uint32), want[f].view(np.uint32)), "TraceRays, any_hit %s: %s" % (any_hit, f)
            assert np.array_equal(bare["ref_idx"], np.where(want["tri_id"] == -1, -1, 0))
            assert (got["tri_id"] >= 0).sum() >= W.least_hits(len(s.tris)), "rays reached"
            excused = int(check_against_fp64_truth(s.tris, rays, got, any_hit=any_hit).sum())  # the model's triangles: nothing of the device's in it
            self.excused = max(self.excused, excused)
            assert excused <= EXCUSED, "%d rays excused by the binary64 truth (any_hit %s)" % (excused, any_hit)

    def image(self, what):
        assert self.p.GetSPP() == self.frames, "GetSPP"
        assert np.array_equal(bits(self.p.ReadResult()), bits(self.picture())), what

    # -- one step --
    def geometry(self, s):
        p = self.p
        name, args, kw = s.call
        keeps = s.op[0] in W.KEEP_THE_IMAGE
        spp, image, parked = p.GetSPP(), p.ReadResult(), None if self.multi else p.GetLookaheadFrames()
        answer = getattr(p, name)(*args, **kw)
        if keeps:  # a bind or an unbind moves no triangle: the accumulation goes on
            assert p.GetSPP() == spp and np.array_equal(bits(p.ReadResult()), bits(image)), "the accumulation after a bind"
            assert self.multi or p.GetLookaheadFrames() == parked, "the frames parked ahead after a bind"
            p.Reset()
        else:
            assert p.GetSPP() == 0, "GetSPP after a geometry call"
            assert self.multi or p.GetLookaheadFrames() == 0, "frames are still parked"
        if s.answer is None:
            assert answer is None
        elif "rebuilt" in s.answer:
            for k in ("built", "refitted", "now", "rebuilt"):
                assert answer[k] == s.answer[k], "the policy's answer: %s is %s, the host's %s" % (k, answer[k], s.answer[k])
            self.info(answer["rebuild"], s.answer["rebuild"])
        else:
            self.info(answer, s.answer)
        tree = self.holds(s)
        assert p.GetTreeCost() == s.cost, "GetTreeCost"
        self.rays(s, tree)
        self.scene_of((tree[0], tree[2], s.tris))
        self.picture(SPP)
        self.trace(SPP)
        if not self.multi and not self.lookahead:
            assert p.GetFusedBounces() == self.fused
        self.image("the image of %d frames after the call" % SPP)
        if p.GetNoiseStats():
            assert (p.ReadBlockSPP()[1] == SPP).all(), "a block is still frozen"

    def info(self, got, want):
        if want is None:
            assert all(v == 0 for v in got.values()), "nothing was rebuilt: %s" % got
        else:
            assert all(got[k] == v for k, v in want.items()) and got["binary_depth"] >= got["levels"] - 1, "RebuildInfo %s, the host's %s" % (got, want)

    def refusal(self, s):
        p = self.p
        name, args, kw = s.call
        before, spp, image = self.read_tree(), p.GetSPP(), p.ReadResult()
        with pytest.raises(N.AdyptError) as e:
            getattr(p, name)(*args, **kw)
        assert e.value.code == s.refused, "refused with %d, not %d: %s" % (e.value.code, s.refused, e.value)
        self.holds(s)
        for a, b in zip(before, self.read_tree()):
            assert same_bytes(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])  # (device against device: NaNs included)
        assert p.GetSPP() == spp and np.array_equal(bits(p.ReadResult()), bits(image)), "the accumulation"

    def disturbance(self, s):
        p = self.p
        kind, k = s.op
        if kind == "trace":
            self.picture(k)
            self.trace(k)
        elif kind == "lookahead":
            p.Reset()
            self.fresh()
            if not self.multi:
                p.SetFramesInFlight(5)
            p.SetLookahead(True)
            self.lookahead = True
            self.picture(1)
            self.trace(1)
            assert self.multi or p.GetLookaheadFrames() == 4, "frames parked ahead"
        elif kind == "adaptive":
            return self.adaptive()
        elif kind == "denoise":
            self.with_noise_stats()
            if self.frames < 2:
                self.picture(SPP)
                self.trace(SPP)
            before = p.ReadResult()
            p.Denoise(temporal=True, follow_motion=True)
            assert np.array_equal(bits(p.ReadResult()), bits(before)), "Denoise changed the image"
        elif kind == "tree_cost":
            assert p.GetTreeCost() == s.cost, "GetTreeCost"
        elif kind == "trace_rays" and not self.multi:
            rays = s.rays()[::8]
            nodes, woop, idx = self.read_tree()[0]
            want = O.trace(O.Scene(nodes, idx, s.tris, self.case.scene.materials, woop=woop), rays, stack_size=PT["stack_size"])
            assert p.TraceRays(rays).tobytes() == want.tobytes(), "TraceRays"
        self.image("the image after the disturbance")

    def with_noise_stats(self):
        p = self.p
        p.SetLookahead(False)
        self.lookahead = False
        if not p.GetNoiseStats():
            p.Reset()
            self.fresh()
            p.SetNoiseStats(True)

    def adaptive(self):
        """Blocks frozen at two frames, the others at four.  One block (32 x 18): it freezes.  Four (two shards): a target between their mean noises
        at two frames, measured on the device first, so that some freeze and some do not; a block holds the oracle's pixels at its own count."""
        p = self.p
        self.with_noise_stats()
        p.Reset()
        self.fresh()
        target = 1e30
        if self.multi:
            p.Trace(True, 2)
            _, total, count = p.ReadBlockNoise()
            mean = np.sort(np.unique(total / count))
            if len(mean) > 1 and mean[len(mean) // 2 - 1] > 0:
                target = float((mean[len(mean) // 2 - 1] * mean[len(mean) // 2]) ** 0.5)
            at_two = total / count <= target
            p.Reset()
        r = p.TraceAdaptive(target, min_spp=2, max_spp=4, check_every=2)
        two = self.picture(2)
        four = self.picture(2)
        _, spp = p.ReadBlockSPP()
        if self.multi:
            assert np.array_equal(spp, np.where(at_two, 2, 4)) and (target == 1e30 or 0 < at_two.sum() < len(spp)), "the blocks frozen: %s" % spp
            print("adaptive: blocks at", spp.tolist())
        else:
            assert r["blocks"] == r["blocks_frozen"] == 1 and spp.tolist() == [2]
        want = four.copy()
        nbx = (self.w + B - 1) // B
        for b, n in enumerate(spp):
            ys, xs = slice(b // nbx * B, (b // nbx + 1) * B), slice(b % nbx * B, (b % nbx + 1) * B)
            want[ys, xs] = (two if n == 2 else four)[ys, xs]
        assert p.GetSPP() == r["spp"] == int(spp.max())
        assert np.array_equal(bits(p.ReadResult()), bits(want)), "the image after TraceAdaptive"


def run(case, steps, variant, sobol_matrices, monkeypatch, seed="-"):
    """the steps on one context; returns the largest number of rays the binary64 truth excused on a step"""
    w = Walker(case, variant, sobol_matrices, monkeypatch)
    try:
        for k, s in enumerate(steps):
            try:
                if k == 0:
                    tree = w.holds(s)
                    w.scene_of((tree[0], tree[2], s.tris))
                elif s.refused is not None:
                    w.refusal(s)
                elif s.category == "disturbance":
                    w.disturbance(s)
                else:
                    w.geometry(s)
            except (AssertionError, N.AdyptError, pytest.fail.Exception) as e:
                raise AssertionError("walk %s (%s), step %d %s, %d triangles: %s\nreplay(%r, %r)" % (
                    seed, variant, k, s.op, len(s.tris), e, [t.op for t in steps[1:k + 1]], steps[0].op[1])) from e
    finally:
        w.p.destroy()
    return w.excused


@pytest.mark.parametrize("seed", W.SEEDS)
def test_walk(seed, sobol_matrices, monkeypatch):
    case, steps = W.steps_of(seed)
    print("walk %d: at most %d rays excused on a step" % (seed, run(case, steps, "default", sobol_matrices, monkeypatch, seed)))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("seed", VARIANT_SEEDS)
def test_walk_variant(seed, variant, sobol_matrices, monkeypatch):
    case, steps = W.steps_of(seed)
    run(case, steps, variant, sobol_matrices, monkeypatch, seed)


# ---- a list of operations as a test of its own: how a failure of a walk is kept ----
@pytest.mark.parametrize("ops", [[("update_all", 1), ("update_keep", 2)], [("update_keep", 2), ("update_keep", 1)]])
def test_reference_cost_is_taken_when_it_is_first_asked_for(ops, sobol_matrices, monkeypatch):
    """README, Refit or rebuild: the policy's reference is measured at the first GetTreeCost() or policy call after the upload, on the tree as it is then.
    Behind a plain UpdateTriangles that is the refitted tree (the walk asks for the cost behind every call); a policy call as the first call measures
    the uploaded tree in front of its own refit.  The first walks' messages, pasted into replay(), were these two lists."""
    case, steps = W.replay(ops, 1)
    assert steps[-1].answer["built"] == steps[1 if ops[0][0] == "update_all" else 0].cost and steps[0].cost != steps[1].cost
    run(case, steps, "default", sobol_matrices, monkeypatch)
