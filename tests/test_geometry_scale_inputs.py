"""What makes the scenes of tests/test_gpu_geometry_scale.py sharp (tests/geometry_scale_scenes.py), held on the CPU: the two outliers are the extremes
of the centroid box on all six faces, the host's tree depends on them, the top count is past the sort's threshold in the installed rocPRIM, and the
split case has more references than that threshold too."""
import numpy as np
import pytest

from tests import geometry_scale_scenes as S
from tests import refit_truth as T
from tests.test_presplit_definition import lib_refs
from tests.test_refit_definition import same_bytes


@pytest.mark.parametrize("n", S.COUNTS)
def test_the_outliers_are_the_extremes_on_every_face(n):
    tris = S.far_ends(n)
    assert len(tris) == n and tris.dtype == T.soup(1).dtype
    soup = T.soup(n, 11)
    assert tris[:n - 2].tobytes() == soup[:n - 2].tobytes(), "everything but the last two is the soup"
    for i in (n - 2, n - 1):  # each keeps its shape
        a, b = tris["p"][i].astype(np.float64), soup["p"][i].astype(np.float64)
        assert np.abs((a - a.mean(axis=0)) - (b - b.mean(axis=0))).max() < 1e-5
    c = tris["p"].astype(np.float64).mean(axis=1)
    assert np.abs(c[n - 2] - S.FAR).max() < 1e-5 and np.abs(c[n - 1] + S.FAR).max() < 1e-5
    in_lo, in_hi = S.centroid_box(tris[:n - 2])
    lo, hi = S.centroid_box(tris)
    print("%d: centroids of [0, n - 2) in %s .. %s, of all in %s .. %s" % (n, in_lo, in_hi, lo, hi))
    assert (lo < in_lo).all() and (in_hi < hi).all(), "on each of the six faces the box without the outliers lies strictly inside"
    # the same of the scene box, whose area sets the thresholds of the pre-split
    p = tris["p"]
    assert (p[n - 1].min(axis=0) < p[:n - 2].min(axis=(0, 1))).all() and (p[n - 2].max(axis=0) > p[:n - 2].max(axis=(0, 1))).all()
    # where they lie: the last partial box of 257 / the second round of threads 0 and 1 / a ragged last workgroup
    if n == 65538:
        assert (n + 255) // 256 == 257 and (n - 2) // 256 == (n - 1) // 256 == 256
    if n == 262146:
        assert (n - 2, n - 1) == (1024 * 256, 1024 * 256 + 1)
    if n == 1048578:
        assert n % 256 == 2 and n % 64 == 2


@pytest.mark.parametrize("n", S.COUNTS)
def test_the_keys_depend_on_the_outliers(n):
    b, _ = S.host_tree(n, "linear")
    plain, _ = S.host_tree(n, "linear", T.soup(n, 11))
    assert len(b.tri_indices) == len(plain.tri_indices) == n
    assert not np.array_equal(b.tri_indices[:n // 2], plain.tri_indices[:n // 2]), "the order of the first half is the same without the outliers"
    assert not same_bytes(b.nodes, plain.nodes)


def test_the_top_count_is_past_the_merge_sort_limit():
    limit, where = S.rocprim_merge_sort_limit()
    if limit is None:
        pytest.skip(where)
    print("merge_sort_limit %d (%s)" % (limit, where))
    assert S.COUNTS[-1] == limit + 2 and S.COUNTS[-2] <= limit


@pytest.mark.parametrize("n", S.COUNTS)
def test_the_split_case_splits(n):
    level, ref_tri, _ = lib_refs(S.far_ends(n), S.SPLIT_BUDGET)
    print("%d triangles, budget %.1f: level %d, %d references" % (n, S.SPLIT_BUDGET, level, len(ref_tri)))
    assert level >= 0 and n < len(ref_tri) <= n + int(S.SPLIT_BUDGET * n)
    if n == S.COUNTS[-1]:
        assert len(ref_tri) > 1048576
        limit, _ = S.rocprim_merge_sort_limit()
        assert limit is None or len(ref_tri) > limit
