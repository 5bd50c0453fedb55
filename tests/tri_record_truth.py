"""The device triangle record (csrc/device/tri_record.hpp) restated in numpy: the 100-byte Triangle -> the 128-byte record and the class byte, and back.
Written from the layout in include/adypt_host.h (adypt_pack_triangles), not from the C++ text."""
import numpy as np

from oracle import oracle_py as O

RECORD_WORDS, SOURCE_WORDS = 32, 25


def material_class(illum, shininess, textured):
    """shade.hpp's shading class per material, vectorised: 3/4 glossy, 1/2 diffuse, 6 dielectric, 5 everything else (the even one of a pair: textured)"""
    illum, textured = np.asarray(illum), np.asarray(textured, dtype=bool)
    glossy = (illum == 2) & (np.asarray(shininess, dtype=np.float32) * np.float32(0.01) > np.float32(0.3))
    diffuse = ~glossy & ((illum == 1) | (illum == 2))
    dielectric = ~glossy & ~diffuse & ((illum == 6) | (illum == 7))
    return np.where(glossy, np.where(textured, 4, 3), np.where(diffuse, np.where(textured, 2, 1), np.where(dielectric, 6, 5))).astype(np.uint8)


def pack(triangles, materials, n_textures):
    """(records uint32 [n, 32], class bytes uint8 [n]) of TRI_DT triangles and MAT_DT materials"""
    t = np.ascontiguousarray(triangles).view(O.TRI_DT).reshape(-1)
    m = np.ascontiguousarray(materials).view(O.MAT_DT).reshape(-1)
    src = t.view(np.uint32).reshape(len(t), SOURCE_WORDS)
    rec = np.zeros((len(t), RECORD_WORDS), dtype=np.uint32)
    rec[:, 0:18] = src[:, 0:18]      # positions and normals
    rec[:, 18] = src[:, 24]          # material id
    rec[:, 20:26] = src[:, 18:24]    # texture coordinates
    matid = t["matid"]
    known = (matid >= 0) & (matid < len(m))
    cls = np.full(len(t), 5, dtype=np.uint8)
    if len(m):
        mm = m[np.where(known, matid, 0)]
        plain = material_class(mm["illum"], mm["shininess"], False)
        rec[:, 19] = np.where(known & ((plain == 3) | (plain == 6)), 1, 0)
        textured = (n_textures != 0) & (mm["dtex"] >= 0) & (mm["dtex"] < n_textures)
        cls = np.where(known, material_class(mm["illum"], mm["shininess"], textured), 5).astype(np.uint8)
    return rec, cls


def unpack(records):
    """the 100-byte triangles (uint8 [n * 100]) of records uint32 [n, 32]"""
    r = np.ascontiguousarray(records).view(np.uint32).reshape(-1, RECORD_WORDS)
    return np.ascontiguousarray(np.concatenate([r[:, 0:18], r[:, 20:26], r[:, 18:19]], axis=1)).view(np.uint8).reshape(-1)
