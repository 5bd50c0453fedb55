"""The walks of tests/geometry_walk.py on the CPU: what they cover, counted, and — from the oracle alone, on the model's host arrays — that the rays
of every step find the triangles that are there (the binary64 brute force of tests/helpers.py, which shares no header with the product).  The GPU
test (tests/test_gpu_geometry_walk.py) makes the same calls on a context and holds it against the same model."""
import numpy as np
import pytest

from adypt_amd import _native as N
from oracle import oracle_py as O
from tests import geometry_walk as W
from tests.helpers import check_against_fp64_truth

STACK = 32   # tests/test_gpu_refit.PT
EXCUSED = 4  # of 4096 rays (0.1 %): the bound of tests/test_gpu_ray_tmin.py


def geometry_pairs(ops):
    """(a, b) for every two geometry operations with nothing but disturbances and refused calls between them, and which b the model refused"""
    _, steps = W.replay(ops)
    out, last = [], None
    for s in steps[1:]:
        if s.category != "geometry":
            continue
        if last is not None:
            out.append((last, s.op[0], s.refused is not None))
        if s.refused is None:
            last = s.op[0]
    return out


def test_every_ordered_pair_of_geometry_kinds_occurs():
    made, refused = set(), set()
    for seed in W.SEEDS:
        for a, b, r in geometry_pairs(W.walk(seed)):
            (refused if r else made).add((a, b))
    every = {(a, b) for a in W.GEOMETRY for b in W.GEOMETRY}
    print("%d walks, %d operations; %d of %d ordered pairs made, %d more stand as a call that must be refused" % (
        len(W.SEEDS), sum(len(W.walk(s)) for s in W.SEEDS), len(made), len(every), len(refused - made)))
    assert made | refused == every
    # a pair is only ever refused where its first call takes away what its second needs
    sketch = W._Sketch(0)
    assert all(sketch.takes_away(a, b) for a, b in refused - made)
    assert len(made) >= len(every) - 64


def test_every_kind_occurs_directly_behind_every_disturbance():
    seen = set()
    for seed in W.SEEDS:
        ops = W.walk(seed)
        seen |= {(d[0], k[0]) for d, k in zip(ops, ops[1:]) if d[0] in W.DISTURBANCES}
    assert seen >= {(d, k) for d in W.DISTURBANCES for k in W.GEOMETRY}


def test_arguments_and_refusals_are_all_drawn():
    calls, refusals, counts = set(), {}, set()
    for seed in W.SEEDS:
        _, steps = W.steps_of(seed)
        assert all(len(s.tris) >= 1 for s in steps)
        counts |= {len(s.tris) for s in steps}
        for s in steps[1:]:
            if s.category == "disturbance":
                continue
            name, args, kw = s.call
            if s.refused is not None:
                refusals.setdefault(s.op[0], set()).add(s.refused)
                continue
            what = [s.op[0]]
            if name == "UpdateTriangles":
                what.append("normals" if len(args) > 2 and args[2] is not None else "positions")
            if name == "PoseVertices":
                what.append("given" if args[1] is not None else "computed")
            what += [kw.get(k) for k in ("method", "radius", "split_budget", "rebuild_above") if k in kw]
            calls.add(tuple(what))
    assert counts >= set(W.COUNTS), "every count is reached"
    for want in [("update_range", "normals"), ("update_range", "positions"), ("update_rebuild", "positions", "ploc", 0.0), ("update_rebuild", "positions", "linear", 0.0),
                 ("update_keep", "positions", "ploc", 1e9), ("rebuild_ploc", "ploc", 8), ("rebuild_ploc", "ploc", W.OTHER_RADIUS), ("rebuild_split", "ploc", 0.3),
                 ("pose_vertices", "given"), ("pose_vertices", "computed"), ("pose_policy", 0.0), ("pose_policy", 1e9), ("pose_vertices_policy", "given", "ploc", 8, 0.0),
                 ("pose_vertices_policy", "computed", "ploc", 8, 1e9)]:
        assert want in calls, want
    assert set(refusals) >= set(W.REFUSALS) | {"pose", "pose_vertices", "pose_morph", "bind_morph"}
    assert refusals["refuse_pose"] == refusals["refuse_pose_vertices"] == {N.E_STATE} and refusals["refuse_update_range"] == refusals["refuse_bind"] == {N.E_INVALID}
    # a policy of 0 rebuilds, one of 1e9 keeps; the reference cost is here the cost in front of the call, there an older one (a policy call that kept its tree before)
    answers = [(s, before) for seed in W.SEEDS for before, s in zip(W.steps_of(seed)[1], W.steps_of(seed)[1][1:]) if s.answer is not None and "rebuilt" in s.answer]
    assert {s.answer["rebuilt"] for s, _ in answers} == {0, 1}
    assert {s.answer["built"] != before.cost for s, before in answers} == {False, True}


def test_replay_of_a_printed_prefix_makes_the_same_arrays():
    """what a failing GPU step prints — the operations up to it and the walk's number — is enough to stand at that step again"""
    seed, k = 4, 21
    _, steps = W.steps_of(seed)
    printed = repr([s.op for s in steps[1:k + 1]])
    _, again = W.replay(eval(printed), steps[0].op[1])
    a, b = steps[k], again[k]
    assert a.op == b.op and a.tris.tobytes() == b.tris.tobytes() and a.nodes.tobytes() == b.nodes.tobytes() and np.array_equal(a.tri_indices, b.tri_indices)
    assert a.rays().tobytes() == b.rays().tobytes() and (a.pose, a.morph, a.mesh, a.answer) == (b.pose, b.morph, b.mesh, b.answer)


@pytest.mark.parametrize("seed", W.SEEDS)
def test_rays_of_every_step_find_the_triangles(seed):
    """On the model's arrays of every step: O.trace reaches at least least_hits() of the step's 4096 rays, and check_against_fp64_truth excuses at most 4
    of them, closest and any hit.  Measured here: no ray excused on any step of 24 walks, at most 1 on walks 2, 23 and 26, at most 2 on walk 5 (printed below)."""
    _, steps = W.steps_of(seed)
    worst, done = 0, None
    for k, s in enumerate(steps):
        if done is not None and s.tris is done.tris and s.nodes is done.nodes and s.tri_indices is done.tri_indices:
            continue  # (the arrays of the step before: nothing to trace again)
        done = s
        osc = O.Scene(s.nodes, s.tri_indices, s.tris, W.T.soup_material(), woop=s.woop)
        rays = s.rays()
        for any_hit in (False, True):
            hits = O.trace(osc, rays, stack_size=STACK, any_hit=any_hit)
            reached = int((hits["tri_id"] >= 0).sum())
            excused = int(check_against_fp64_truth(s.tris, rays, hits, any_hit=any_hit).sum())
            worst = max(worst, excused)
            what = "walk %d step %d %s, %d triangles, any_hit %s: %d rays reached, %d excused" % (seed, k, s.op, len(s.tris), any_hit, reached, excused)
            assert reached >= W.least_hits(len(s.tris)), what
            assert excused <= EXCUSED, what
    print("walk %d: at most %d rays excused on a step" % (seed, worst))
