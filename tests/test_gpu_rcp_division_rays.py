"""-m gpu: rays whose direction components lie in [2^126, 2^128) through the real traversal kernels.  The ray setup normalises the direction
and takes 1 / d, both with rcp_ieee (canon_math.hpp), which leaves v_rcp_f32 + Newton for the division sequence at biased exponents 0, 253,
254 and 255.  No ray of any other test gets there; these do twice: the squared length overflows, so the reciprocal is taken of +inf, the
normalised direction is (+-0, +-0, +-0) and its reciprocal +-inf.  On the CPU such a ray visits a large part of the BVH and hits nothing, so
the parity with the oracle is in the node and triangle counts, the visit hash and the stack depth: asserted non-trivial on the oracle's side
first.  (No such ray can hit: one component of 2^64 or more already makes the length infinite, and the product with its reciprocal 0 turns the
ordinary components into +-0 as well.  N_MIXED rays with one or two huge components ride along to show it; only the instrumented kernel's counts
tell whether the slab test read the right planes.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_py as O  # noqa: E402
from tests.helpers import bits, golden_scene, oracle_scene_from_golden  # noqa: E402
from tests.test_gpu_parity import golden_tracer  # noqa: E402

N_RAYS = 4096
N_MIXED = 512
STACK = 32
TMINS = np.float32([0.0, -1.0, 1e-4])


def huge_direction_rays(tris, n, seed):
    """(n, 8) rays from inside the scene's bounds; every direction component has biased exponent 253 or 254, any mantissa, either sign;
    tmin cycles through TMINS from ray to ray."""
    rs = np.random.RandomState(seed)
    p = tris["p"].reshape(-1, 3)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = rs.uniform(p.min(0), p.max(0), size=(n, 3))
    rays[:, 3] = TMINS[np.arange(n) % len(TMINS)]
    word = (rs.randint(0, 2, size=(n, 3)).astype(np.uint32) << 31) | (rs.randint(253, 255, size=(n, 3)).astype(np.uint32) << 23) | \
        rs.randint(0, 1 << 23, size=(n, 3)).astype(np.uint32)
    word[:8] = (word[:8] & np.uint32(0x80000000)) | np.uint32([[0x7e800000] * 3, [0x7f7fffff] * 3, [0x7e800000, 0x7f7fffff, 0x7f000000],
                                                               [0x7f000000] * 3, [0x7e800001] * 3, [0x7effffff] * 3, [0x7f000001] * 3,
                                                               [0x7f7fffff, 0x7e800000, 0x7e800000]])  # 2^126, the largest float, 2^127 and neighbours
    rays[:, 4:7] = word.view(np.float32)
    return rays


def mixed_direction_rays(tris, n, seed):
    """the same, but only one or two components of each direction are huge: the others are ordinary (they come out of normalize as +-0 too)"""
    rs = np.random.RandomState(seed)
    rays = huge_direction_rays(tris, n, seed + 1)
    ordinary = rs.normal(size=(n, 3)).astype(np.float32)
    keep_huge = np.zeros((n, 3), bool)
    keep_huge[np.arange(n), rs.randint(0, 3, size=n)] = True
    keep_huge[np.arange(n), rs.randint(0, 3, size=n)] |= rs.uniform(size=n) < 0.5
    rays[:, 4:7] = np.where(keep_huge, rays[:, 4:7], ordinary)
    return rays


@pytest.mark.parametrize("name", ["tiny0", "tiny1"])
def test_rays_with_huge_directions_bit_exact(name):
    _, _, nodes, tris, _, _ = golden_scene(name)
    rays = huge_direction_rays(tris, N_RAYS, 41)
    d = np.abs(rays[:, 4:7])
    assert (d >= np.float32(2.0 ** 126)).all() and np.isfinite(d).all() and set(rays[:, 3].tolist()) == set(TMINS.tolist())
    mixed = mixed_direction_rays(tris, N_MIXED, 43)
    n_huge = (np.abs(mixed[:, 4:7]) >= np.float32(2.0 ** 126)).sum(1)
    assert set(n_huge.tolist()) == {1, 2} and ((mixed[:, 4:7] < 0) & (np.abs(mixed[:, 4:7]) < 10)).any(1).sum() > 100
    rays = np.concatenate([rays, mixed])
    osc = oracle_scene_from_golden(name)
    pt = golden_tracer(name, stack=STACK)
    for any_hit in (False, True):
        oh = O.trace(osc, rays, STACK, any_hit=any_hit)
        # not vacuous: the oracle walks the tree for every one of these rays (tiny0: 51.1 of 123 nodes and 351 triangle tests per ray) and hits nothing
        assert (oh["tri_id"] == -1).all() and (oh["ref_idx"] == -1).all()
        assert oh["nodes"].min() >= 1 and oh["nodes"].mean() > 0.3 * len(nodes) and oh["tris"].mean() > 100 and oh["max_depth"].max() >= 3
        assert len(np.unique(oh["hash"])) > 8
        print("%s any_hit=%s: %.1f nodes, %.1f triangle tests per ray, max depth %d" % (name, any_hit, oh["nodes"].mean(), oh["tris"].mean(),
                                                                                      oh["max_depth"].max()))
        gh = pt.TraceRays(rays, with_stats=True, any_hit=any_hit)
        assert gh.tobytes() == oh.tobytes(), "instrumented kernel, any_hit=%s: %d records differ (nodes %d, tris %d, hash %d, depth %d)" % (
            any_hit, (gh != oh).sum(), (gh["nodes"] != oh["nodes"]).sum(), (gh["tris"] != oh["tris"]).sum(), (gh["hash"] != oh["hash"]).sum(),
            (gh["max_depth"] != oh["max_depth"]).sum())
        g2 = pt.TraceRays(rays, with_stats=False, any_hit=any_hit)
        assert np.array_equal(g2["tri_id"], oh["tri_id"]), "kernel without statistics, any_hit=%s: triangles" % any_hit
        for k in ("u", "v", "t"):
            assert np.array_equal(bits(g2[k]), bits(oh[k])), "kernel without statistics, any_hit=%s: %s" % (any_hit, k)
        assert (g2["ref_idx"] == -1).all()
