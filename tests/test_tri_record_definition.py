"""The device triangle record has ONE definition (csrc/device/tri_record.hpp), which the host's adypt_pack_triangles and the device's k_pack_triangles both
compile: here the host's bytes are held against the numpy restatement (tests/tri_record_truth.py); tests/test_gpu_set_triangles.py holds the device's
against the host's.  Also: the new symbols of the C-ABI with their argument types, and the command line's --build."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from adypt_amd import api, scenes, _native as N
from oracle import oracle_py as O
from tests import refit_truth as T
from tests import tri_record_truth as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lib_pack(tris, mats, n_textures, want_classes=True):
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    m = np.ascontiguousarray(mats).view(np.uint8).reshape(-1)
    n = len(t) // 100
    rec = np.full((n, 32), 0xdeadbeef, dtype=np.uint32)
    cls = np.full(n, 0xee, dtype=np.uint8)
    r = N.lib.adypt_pack_triangles(t.ctypes.data, n, m.ctypes.data if len(m) else None, len(m) // 64, n_textures, rec.ctypes.data, cls.ctypes.data if want_classes else None)
    assert r == N.ADYPT_OK
    return rec, cls


def class_soup():
    """300 triangles over a material table in which every class occurs (3 and 6 among them), one id of -1 and one of n_mats; two "textures\""""
    m = np.zeros(8, dtype=O.MAT_DT)
    m["dtex"], m["etex"], m["stex"] = (-1, 0, -1, 1, -1, 2, -1, 0), -1, -1
    m["illum"] = (2, 2, 2, 2, 6, 7, 4, 1)
    m["shininess"] = (10.0, 10.0, 80.0, 80.0, 5.0, 90.0, 50.0, 30.000002)
    m["kd"], m["dissolve"], m["ior"] = (0.7, 0.6, 0.5), 1.0, 1.5
    t = T.soup(300, 13)
    t["matid"] = np.arange(300) % 8
    t["matid"][17], t["matid"][250] = -1, 8
    t["tc"] = np.random.RandomState(2).uniform(-2, 2, size=t["tc"].shape).astype(np.float32)
    return t, m, 2


def inputs(name, cache):
    if name == "soup":
        return class_soup()
    spec = scenes.make_scene(name, cache, width=32, height=18)
    cfg = api.InstanceConfig()
    assert cfg.LoadFromFile(spec.config_path), api.InstanceConfig.last_error()
    s = api.Scene()
    assert s.LoadFromFile(cfg.m_obj_filename)
    return np.array(s.triangles).view(O.TRI_DT), np.array(s.materials).view(O.MAT_DT), len(s.textures)


@pytest.mark.parametrize("name", ["tiny0", "tiny1", "tiny2", "soup"])
def test_library_equals_numpy(name, scene_cache):
    tris, mats, n_tex = inputs(name, scene_cache)
    rec, cls = lib_pack(tris, mats, n_tex)
    want_rec, want_cls = R.pack(tris, mats, n_tex)
    assert rec.tobytes() == want_rec.tobytes(), "the 128-byte records"
    assert cls.tobytes() == want_cls.tobytes(), "the class bytes"
    assert R.unpack(rec).tobytes() == np.ascontiguousarray(tris).tobytes(), "the records unpack to the 100 input bytes"
    assert not rec[:, 26:].any() and set(np.unique(rec[:, 19])) <= {0, 1}
    assert lib_pack(tris, mats, n_tex, want_classes=False)[0].tobytes() == want_rec.tobytes()  # (classes_out may be NULL)
    if name == "soup":
        assert set(np.unique(rec[:, 19])) == {0, 1}, "both values of the class word occur"
        plain = R.material_class(mats["illum"], mats["shininess"], False)
        assert {3, 6} <= set(plain) and set(cls) == {1, 2, 3, 4, 5, 6}
        assert rec[17, 19] == 0 and rec[250, 19] == 0 and cls[17] == 5 and cls[250] == 5  # ids outside [0, n_mats)
        assert rec[17, 18] == 0xffffffff and rec[250, 18] == 8  # ... which stay in the record as they are
        known = (tris["matid"] >= 0) & (tris["matid"] < 8)
        assert np.array_equal(rec[:, 19] == 1, known & np.isin(tris["matid"], (2, 3, 4, 5)))  # glossy with and without a texture, both dielectrics
        # without textures no class is a textured one
        assert set(lib_pack(tris, mats, 0)[1]) == {1, 3, 5, 6}


def test_refusals():
    t, m, _ = class_soup()
    rec = np.zeros((300, 32), np.uint32)
    assert N.lib.adypt_pack_triangles(None, 300, m.ctypes.data, 8, 0, rec.ctypes.data, None) == N.E_INVALID
    assert N.lib.adypt_pack_triangles(t.ctypes.data, -1, m.ctypes.data, 8, 0, rec.ctypes.data, None) == N.E_INVALID
    assert N.lib.adypt_pack_triangles(t.ctypes.data, 300, None, 8, 0, rec.ctypes.data, None) == N.E_INVALID
    assert N.lib.adypt_pack_triangles(t.ctypes.data, 0, None, 0, 0, rec.ctypes.data, None) == N.ADYPT_OK


NEW_SYMBOLS = {
    "adypt_pack_triangles": (C.c_int, 7),
    "adypt_set_triangles": (C.c_int, 8),
    "adypt_create_from_triangles": (C.c_int, 7),
    "adypt_get_triangle_count": (C.c_int64, 1),
    "adypt_read_triangle_records": (C.c_int, 2),
    "adypt_multi_set_triangles": (C.c_int, 8),
    "adypt_create_multi_from_triangles": (C.c_int, 9),
}


def test_new_symbols_in_header_and_binding():
    text = open(os.path.join(ROOT, "include", "adypt_hip.h")).read() + open(os.path.join(ROOT, "include", "adypt_host.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (restype, n_args) in NEW_SYMBOLS.items():
        m = re.search(r"\b(int64_t|int)\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, "%s is not declared" % name
        assert len(m.group(2).split(",")) == n_args, name
        assert (m.group(1) == "int64_t") == (restype is C.c_int64), name
        res, args = N._SIGS[name]
        assert name in N.EXPORTS and res is restype and len(args) == n_args, name
        assert hasattr(C.CDLL(N.LIB_PATH), name)
    assert N._SIGS["adypt_set_triangles"][1] == [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(N.BvhParams), C.c_int, C.c_int, C.c_double, C.POINTER(N.RebuildInfo)]
    assert N._SIGS["adypt_create_from_triangles"][1][2:] == [C.POINTER(N.BvhParams), C.c_int, C.c_int, C.c_double, C.POINTER(N.RebuildInfo)]
    assert N.lib.adypt_abi_version() == 4
    # without a context nothing is touched
    assert N.lib.adypt_set_triangles(None, None, 0, None, 1, 8, 0.0, None) == N.E_INVALID
    assert N.lib.adypt_get_triangle_count(None) == N.E_INVALID and N.lib.adypt_read_triangle_records(None, None) == N.E_INVALID


def test_create_from_triangles_refuses_before_touching_a_device():
    tris, mats = T.soup(9, 5), T.soup_material()
    hs = api.HipScene()
    hs.Initialize(api.Scene.FromArrays(tris, mats))
    for kw, word in ((dict(method="ploc", radius=0), "radius"), (dict(method="ploc", radius=33), "radius"), (dict(split_budget=1.5), "budget"),
                     (dict(method="linear", split_budget=0.25), "budget")):
        with pytest.raises(N.AdyptError) as e:
            api.HipPathTracer().Initialize(api.InstanceConfig().pt_params(), hs, 32, 18, **kw)
        assert e.value.code == N.E_INVALID and word in str(e.value), kw
    with pytest.raises(ValueError):
        api.HipPathTracer().Initialize(api.InstanceConfig().pt_params(), hs, 32, 18, method="sbvh")
    # a description that names a tree is adypt_create's
    d, keep = api._scene_desc(hs, 32, 18)
    node = np.zeros(80, np.uint8)
    d.nodes, d.n_nodes = node.ctypes.data, 1
    h = C.c_void_p()
    assert N.lib.adypt_create_from_triangles(C.byref(h), C.byref(d), None, 1, 8, 0.0, None) == N.E_INVALID and not h
    assert b"names a tree" in N.lib.adypt_last_error(None)


CLI = os.path.join(ROOT, "adypt_amd", "adypt_hip")


@pytest.mark.parametrize("args", [["--build", "gpu", "--rebuild"], ["--build", "cpu"], ["--build", "sbvh"], ["--build"]])
def test_command_line_refuses(args, scene_cache):
    spec = scenes.make_scene("tiny2", scene_cache, width=32, height=18)
    r = subprocess.run([CLI, spec.config_path] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr)
