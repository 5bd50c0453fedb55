"""An indexed mesh posed by its vertices, on the host: adypt_mesh_normals and adypt_mesh_triangles (csrc/device/mesh.hpp) against the numpy restatement
(tests/mesh_truth.py) bit for bit, adypt_weld_triangles and its round trip, a crease, the length of a computed normal, and what is refused.  No GPU."""
import numpy as np
import pytest

from adypt_amd import _native as N
from adypt_amd import api, scenes
from oracle import oracle_py as O
from tests import mesh_truth as M
from tests import refit_truth as T
from tests.helpers import bits
from tests.test_pose_definition import same_triangles

MESHES = {
    "fan1": lambda: M.fan(1), "fan63": lambda: M.fan(63), "fan64": lambda: M.fan(64), "fan65": lambda: M.fan(65), "fan256": lambda: M.fan(256),
    "fan257": lambda: M.fan(257), "fan300": lambda: M.fan(300), "grid": lambda: M.grid(40, 32), "pair": M.opposite_pair,
    "unreferenced": M.with_unreferenced, "doubled": M.with_doubled_index,
}
_tiny0 = []


def tiny0(cache):
    if not _tiny0:
        spec = scenes.make_scene("tiny0", cache, width=32, height=18)
        cfg = api.InstanceConfig()
        assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
        scene = api.Scene()
        assert scene.LoadFromFile(cfg.m_obj_filename)
        t = np.array(scene.triangles).view(O.TRI_DT)
        t.setflags(write=False)
        _tiny0.append(t)
    return _tiny0[0]


def check_against_numpy(tris, idx, p):
    nv = len(p)
    ref = M.referenced(idx, nv)
    for pos in (p, M.deform(p, 1)):
        got = api.mesh_normals(idx, pos)
        want = M.normals(idx, pos)
        assert np.array_equal(bits(got), bits(want))
        assert not got[~ref].any()
        given = M.some_normals(nv)
        assert same_triangles(api.mesh_triangles(tris, idx, pos), M.triangles(tris, idx, pos))
        assert same_triangles(api.mesh_triangles(tris, idx, pos, given), M.triangles(tris, idx, pos, given))
    t = api.mesh_triangles(tris, idx, p).view(O.TRI_DT)
    for f in set(tris.dtype.names) - {"p", "n"}:
        assert np.array_equal(np.ascontiguousarray(t[f]).view(np.uint8), np.ascontiguousarray(tris[f]).view(np.uint8)), f


@pytest.mark.parametrize("name", sorted(MESHES))
def test_normals_and_triangles_equal_numpy(name):
    idx, p = MESHES[name]()
    if name.startswith("fan"):
        k = int(name[3:])
        assert len(idx) == k and len(p) == k + 2 and np.bincount(idx.ravel())[0] == k
    check_against_numpy(M.rest_triangles(idx, p), idx, p)


def test_the_generators_are_what_they_say():
    idx, p = M.grid(40, 32)
    valence = np.bincount(idx.ravel(), minlength=len(p)).reshape(33, 41)
    assert len(idx) == 2 * 40 * 32 and (valence[1:-1, 1:-1] == 6).all()
    idx, p = M.opposite_pair()
    acc, _ = M.sums(idx, p)
    n, ok = M.normalise(acc)
    assert not acc.any() and not ok.any() and np.array_equal(bits(n), bits(acc))  # every sum cancels: the normal is the sum, signs of zero included
    assert np.array_equal(bits(api.mesh_normals(idx, p)), bits(acc))
    idx, p = M.with_unreferenced()
    assert not M.referenced(idx, len(p))[3] and M.referenced(idx, len(p)).sum() == len(p) - 1
    idx, p = M.with_doubled_index()
    assert (idx[-1] == (1, 1, 2)).all() and not M.faces(idx, p)[-1].any()


def test_the_order_of_the_sum_is_the_lists():
    """(1e8 + -1e8) + 1 = 1 in binary32 and (1e8 + 1) + -1e8 = 0: vertex 0's three face vectors along z are added in ascending triangle order"""
    p = np.array([[0, 0, 0], [1e4, 0, 0], [0, 1e4, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    results = []
    for order in ([0, 1, 2], [0, 2, 1]):
        idx = np.array([[0, 1, 2], [0, 2, 1], [0, 3, 4]], np.int32)[order]
        acc, _ = M.sums(idx, p)
        assert np.array_equal(bits(api.mesh_normals(idx, p)), bits(M.normalise(acc)[0]))
        results.append(float(acc[0, 2]))
    assert results == [1.0, 0.0]


def test_welded_tiny0_equals_numpy(scene_cache):
    tris = tiny0(scene_cache)
    idx, p, n = api.weld_triangles(tris)
    assert len(p) < 3 * len(tris)  # (vertices are shared)
    check_against_numpy(tris, idx, p)


@pytest.mark.parametrize("name", ["tiny0", "soup"])
def test_weld_round_trip(name, scene_cache):
    tris = tiny0(scene_cache) if name == "tiny0" else T.soup(5000)
    idx, p, n = api.weld_triangles(tris)
    assert idx.shape == (len(tris), 3) and idx.dtype == np.int32 and p.shape == n.shape == (idx.max() + 1, 3)
    if name == "soup":
        assert (np.bincount(idx.ravel()) == 1).all() and len(p) == 3 * len(tris)  # every vertex has valence 1
    # numbered in order of first appearance over corners in ascending 3 t + c
    first = np.unique(idx.ravel(), return_index=True)[1]
    assert (np.diff(first) > 0).all()
    assert np.array_equal(bits(p), bits(tris["p"].reshape(-1, 3)[first])) and np.array_equal(bits(n), bits(tris["n"].reshape(-1, 3)[first]))
    assert same_triangles(api.mesh_triangles(tris, idx, p, n), tris)
    # a vertex is its 24 bytes: no two alike
    keys = np.concatenate([bits(p), bits(n)], axis=1)
    assert len(np.unique(keys, axis=0)) == len(keys)


def test_weld_keeps_a_crease():
    idx, p = M.grid(2, 1)
    smooth = M.rest_triangles(idx, p)
    assert len(api.weld_triangles(smooth)[1]) == len(p)  # one vertex per position
    crease = smooth.copy()
    crease["n"][1, 0] = (0.0, 0.0, 1.0)  # a corner that triangles 0 and 2 share keeps its position and gets another normal
    i1, p1, n1 = api.weld_triangles(crease)
    assert len(p1) == len(p) + 1
    a = i1[1, 0]
    twins = [v for v in range(len(p1)) if np.array_equal(bits(p1[v]), bits(p1[a]))]
    assert len(twins) == 2 and not np.array_equal(bits(n1[twins[0]]), bits(n1[twins[1]]))
    assert np.array_equal(bits(n1[a]), bits(np.array([0.0, 0.0, 1.0], np.float32)))
    assert same_triangles(api.mesh_triangles(crease, i1, p1, n1), crease)
    # the computed normals then sum over each side of the crease on its own
    assert np.bincount(i1.ravel())[a] == 1
    # vertices are compared as bits: -0.0 is not +0.0
    zero = smooth.copy()
    zero["p"][..., 1][idx == idx[1, 0]] = 0.0
    assert len(api.weld_triangles(zero)[1]) == len(p)
    zero["p"][1, 0, 1] = -0.0
    assert len(api.weld_triangles(zero)[1]) == len(p) + 1
    assert same_triangles(api.mesh_triangles(zero, *api.weld_triangles(zero)), zero)


def test_computed_normals_have_unit_length(scene_cache):
    """n = acc / sqrtf(len2): len2 carries at most three roundings per term (3 u relative, all terms positive), its root half of that and one more, the
    division one more: the length is within 3.5 u = 1.75 ulp of 1, u = 2^-24, ulp = 2^-23.  Held to 2 ulp."""
    tris = tiny0(scene_cache)
    meshes = [M.grid(40, 32), M.fan(300), api.weld_triangles(tris)[:2]]
    for idx, p in meshes:
        acc, _ = M.sums(idx, p)
        _, ok = M.normalise(acc)
        n = api.mesh_normals(idx, p)[ok].astype(np.float64)
        assert ok.sum() > 0.9 * len(p)
        assert np.abs(np.sqrt((n * n).sum(axis=1)) - 1.0).max() <= 2 * 2.0 ** -23


def test_refusals_leave_the_output_untouched():
    idx, p = M.fan(5)
    nv, nt = len(p), len(idx)
    tris = M.rest_triangles(idx, p)
    tin = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    nrm = M.some_normals(nv)
    out_n = np.full((nv, 3), 7.0, np.float32)
    out_t = np.full(100 * nt, 7, np.uint8)
    L = N.lib

    def bad(a, at, value):
        a = a.copy()
        a[at] = value
        return a

    def normals_call(i=idx, n_tris=nt, n_vertices=nv, pos=p, out=out_n):
        return L.adypt_mesh_normals(None if i is None else i.ctypes.data, n_tris, n_vertices, None if pos is None else pos.ctypes.data, None if out is None else out.ctypes.data)

    def triangles_call(t=tin, i=idx, n_tris=nt, n_vertices=nv, pos=p, n=nrm, out=out_t):
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.adypt_mesh_triangles(ptr(t), n_tris, ptr(i), n_vertices, ptr(pos), ptr(n), ptr(out))

    refusals = [
        ("indices is null", lambda: normals_call(i=None)),
        ("positions is null", lambda: normals_call(pos=None)),
        ("the output is null", lambda: normals_call(out=None)),
        ("a negative n_tris", lambda: normals_call(n_tris=-1)),
        ("no vertices", lambda: normals_call(n_vertices=0)),
        ("too many vertices", lambda: normals_call(n_vertices=2 ** 31)),
        ("an index below 0", lambda: normals_call(i=bad(idx, (2, 1), -1))),
        ("an index past the last", lambda: normals_call(i=bad(idx, (nt - 1, 2), nv))),
        ("fewer vertices than the indices name", lambda: normals_call(n_vertices=nv - 1)),
        ("a NaN position", lambda: normals_call(pos=bad(p, (3, 0), np.nan))),
        ("an infinite position", lambda: normals_call(pos=bad(p, (nv - 1, 2), -np.inf))),
        ("triangles_in is null", lambda: triangles_call(t=None)),
        ("triangles_out is null", lambda: triangles_call(out=None)),
        ("indices is null (triangles)", lambda: triangles_call(i=None)),
        ("positions is null (triangles)", lambda: triangles_call(pos=None)),
        ("an index past the last (triangles)", lambda: triangles_call(i=bad(idx, (0, 0), nv))),
        ("too many vertices (triangles)", lambda: triangles_call(n_vertices=2 ** 31)),
        ("a NaN position (triangles)", lambda: triangles_call(pos=bad(p, (0, 1), np.nan))),
        ("a NaN given normal", lambda: triangles_call(n=bad(nrm, (1, 1), np.nan))),
        ("an infinite given normal", lambda: triangles_call(n=bad(nrm, (nv - 1, 0), np.inf))),
    ]
    for what, call in refusals:
        assert call() == N.E_INVALID, what
        assert (out_n == 7.0).all() and (out_t == 7).all(), what
    assert L.adypt_weld_triangles(None, nt, None, None, None) == N.E_INVALID and L.adypt_weld_triangles(tin.ctypes.data, -1, None, None, None) == N.E_INVALID
    assert L.adypt_weld_triangles(tin.ctypes.data, nt, None, None, None) == nv  # the size alone
    with pytest.raises(N.AdyptError) as e:
        api.mesh_normals(bad(idx, (0, 0), nv), p)
    assert e.value.code == N.E_INVALID and "index" in str(e.value)
    # and all is well with good arguments
    assert normals_call() == N.ADYPT_OK and triangles_call() == N.ADYPT_OK
    assert np.array_equal(bits(out_n), bits(M.normals(idx, p))) and same_triangles(out_t, M.triangles(tris, idx, p, nrm))
