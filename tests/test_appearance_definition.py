"""The material table and the texture arena have ONE definition (csrc/device/appearance.hpp), which the host's adypt_pack_appearance and the device's
adypt_set_materials / k_pack_texels both compile: here the host's bytes are held against the numpy restatement (tests/appearance_truth.py);
tests/test_gpu_appearance.py holds the device's against both and against what adypt_create makes of the same arrays.  Also: the new symbols of the
C-ABI with their argument types."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from adypt_amd import api, _native as N
from oracle import oracle_py as O
from tests import appearance_truth as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (w, h): a single texel, rows shorter than a wave, heights that make the wrap word matter, the 256-pixel tile of k_pack_texels from below, at it and above
# it, and one of several tiles whose rows straddle them
SIZES = [(1, 1), (2, 1), (3, 1), (1, 3), (5, 3), (255, 2), (256, 1), (257, 3), (300, 70)]


def texture(w, h, seed):
    """uint8 [h, w, 3] in which no two rows are alike (a wrong wrap texel shows) and no byte plane equals another"""
    t = np.random.RandomState(1000 + seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    t[:, 0, 0] = (np.arange(h) * 37 + 11) % 256  # every row's first texel differs from the rows' around it
    return t


def textures_of(sizes, seed=0):
    return [texture(w, h, seed + i) for i, (w, h) in enumerate(sizes)]


def materials(dtex):
    m = np.zeros(len(dtex), dtype=O.MAT_DT)
    m["dtex"], m["etex"], m["stex"] = dtex, -1, -1
    m["illum"] = np.arange(len(dtex)) % 8
    m["shininess"] = np.linspace(1.0, 200.0, len(dtex)).astype(np.float32) if len(dtex) else 0
    m["kd"], m["dissolve"], m["ior"] = (0.7, 0.6, 0.5), 1.0, 1.5
    return m


def same(got, want):
    for g, w, what in zip(got, want, ("records", "texels", "descriptors")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what


def test_no_textures():
    m = materials([-1, 0, 5, -7])
    got = api.pack_appearance(m, [])
    same(got, A.pack(m, []))
    assert not got[0][:, 16:].any() and got[1].size == 0 and got[2].shape == (0, 4)


def test_no_materials():
    tex = textures_of([(5, 3), (1, 1)])
    got = api.pack_appearance(np.zeros(0, np.uint8), tex)
    same(got, A.pack(np.zeros(0, np.uint8), tex))
    assert got[0].shape == (0, 20) and got[1].size == 6 * 3 + 2
    same(api.pack_appearance(np.zeros(0, np.uint8), []), A.pack(np.zeros(0, np.uint8), []))


def test_every_size_in_one_call():
    tex = textures_of(SIZES)
    n = len(tex)
    m = materials([-1, 0, n - 1, n, 3, -2, 2 ** 31 - 1])
    got = api.pack_appearance(m, tex)
    same(got, A.pack(m, tex))
    rec, texels, desc = got
    assert rec[0, 16:].tolist() == [0, 0, 0, 0] and rec[3, 16:].tolist() == [0, 0, 0, 0], "dtex = -1 and dtex = n_textures have no descriptor"
    assert rec[1, 16:].tolist() == [0, 1, 1, 0] and rec[2, 16:].tolist() == desc[n - 1].tolist()
    assert (desc[:, 0] % 2).any() and not (desc[:, 0] % 2).all(), "bases at odd and at even offsets"
    assert (texels >> 24 == 0xff).all()
    # the wrap word is its own row's first, not the next row's
    o, w, h, _ = desc[4]
    rows = texels[o:o + (w + 1) * h].reshape(h, w + 1)
    assert np.array_equal(rows[:, w], rows[:, 0]) and len(set(rows[:, 0].tolist())) == h


@pytest.mark.parametrize("size", SIZES)
def test_each_size_alone(size):
    tex = textures_of([size], seed=7)
    m = materials([0, 1])
    same(api.pack_appearance(m, tex), A.pack(m, tex))


def test_several_orders_move_the_bases():
    for order in ([4, 0, 7, 2], [7, 7, 1, 8, 0], [8, 3]):
        tex = textures_of([SIZES[i] for i in order], seed=3)
        m = materials(list(range(-1, len(order) + 1)))
        same(api.pack_appearance(m, tex), A.pack(m, tex))


def test_sizes_first_then_bytes():
    tex = textures_of([(5, 3), (2, 1)])
    arr = (N.Texture * 2)()
    for i, t in enumerate(tex):
        arr[i].width, arr[i].height, arr[i].rgb = t.shape[1], t.shape[0], t.ctypes.data
    assert N.lib.adypt_pack_appearance(None, 0, C.addressof(arr), 2, None, None, None) == 6 * 3 + 3 * 1


def test_refusals():
    t = texture(4, 4, 0)
    arr = (N.Texture * 1)()
    out = np.zeros(64, np.uint32)
    m = materials([0])

    def call(mats, n_mats, tex, n_tex):
        return N.lib.adypt_pack_appearance(mats, n_mats, tex, n_tex, None, out.ctypes.data, None)
    arr[0].width, arr[0].height, arr[0].rgb = 4, 4, t.ctypes.data
    assert call(m.ctypes.data, 1, C.addressof(arr), 1) == 20
    assert call(None, 1, C.addressof(arr), 1) == N.E_INVALID
    assert call(m.ctypes.data, -1, C.addressof(arr), 1) == N.E_INVALID
    assert call(m.ctypes.data, 1, None, 1) == N.E_INVALID
    assert call(m.ctypes.data, 1, C.addressof(arr), -1) == N.E_INVALID
    for w, h, rgb in ((0, 4, t.ctypes.data), (4, 0, t.ctypes.data), (-3, 4, t.ctypes.data), (4, 4, None), (2 ** 16, 2 ** 15, t.ctypes.data)):
        arr[0].width, arr[0].height, arr[0].rgb = w, h, rgb
        assert N.lib.adypt_pack_appearance(m.ctypes.data, 1, C.addressof(arr), 1, None, None, None) == N.E_INVALID, (w, h)  # (2^16 x 2^15: more than 2^31 words)
    with pytest.raises(N.AdyptError):
        api.pack_appearance(m, [np.zeros((0, 4, 3), np.uint8)])
    with pytest.raises(ValueError):
        api.pack_appearance(m, [np.zeros((4, 4), np.uint8)])
    with pytest.raises(ValueError):
        api.pack_appearance(np.zeros(65, np.uint8), [])


NEW_SYMBOLS = {
    "adypt_pack_appearance": (C.c_int64, 7),
    "adypt_set_materials": (C.c_int, 5),
    "adypt_update_texture": (C.c_int, 5),
    "adypt_set_triangle_attributes": (C.c_int, 5),
    "adypt_read_material_records": (C.c_int, 2),
    "adypt_read_texels": (C.c_int, 2),
    "adypt_get_appearance": (C.c_int, 2),
    "adypt_multi_set_materials": (C.c_int, 5),
    "adypt_multi_update_texture": (C.c_int, 5),
    "adypt_multi_set_triangle_attributes": (C.c_int, 5),
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
    assert N.lib.adypt_abi_version() == 4
    assert C.sizeof(N.AppearanceInfo) == 48
    # without a context nothing is touched
    assert N.lib.adypt_set_materials(None, None, 0, None, -1) == N.E_INVALID and N.lib.adypt_update_texture(None, 0, None, 1, 1) == N.E_INVALID
    assert N.lib.adypt_set_triangle_attributes(None, 0, 0, None, None) == N.E_INVALID and N.lib.adypt_get_appearance(None, None) == N.E_INVALID
    assert N.lib.adypt_read_material_records(None, None) == N.E_INVALID and N.lib.adypt_read_texels(None, None) == N.E_INVALID
    for cls in (api.HipPathTracer, api.MultiPathTracer):
        for method in ("SetMaterials", "UpdateTexture", "SetTriangleAttributes", "ReadMaterialRecords", "ReadTexels", "GetAppearance"):
            assert callable(getattr(cls, method))
