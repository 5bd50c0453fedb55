"""The device's material table and texture arena (csrc/device/appearance.hpp) restated in numpy.  Written from the layout in include/adypt_host.h
(adypt_pack_appearance), not from the C++ text:
    record   a material's 64 bytes, then (texel offset, w, h, 0) of its diffuse texture where 0 <= dtex < n_textures, else 16 zero bytes
    arena    texture after texture, back to back; each h rows of w + 1 words r | g << 8 | b << 16 | 0xff000000, a row's last word a copy of its first
    desc     (offset, w, h, 0) per texture"""
import numpy as np

MAT_WORDS, RECORD_WORDS = 16, 20


def describe(textures):
    """int32 [n, 4] descriptors and the arena's length in words"""
    desc, at = np.zeros((len(textures), 4), dtype=np.int32), 0
    for i, t in enumerate(textures):
        h, w = t.shape[:2]
        desc[i] = (at, w, h, 0)
        at += (w + 1) * h
    assert at < 2 ** 31
    return desc, at


def arena(textures):
    """uint32 [words] of uint8 [h, w, 3] images"""
    parts = []
    for t in textures:
        t = np.asarray(t, dtype=np.uint8).astype(np.uint32)
        rows = t[:, :, 0] | t[:, :, 1] << 8 | t[:, :, 2] << 16 | np.uint32(0xff000000)
        parts.append(np.concatenate([rows, rows[:, :1]], axis=1).reshape(-1))
    return np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, dtype=np.uint32)


def records(materials, textures):
    """uint32 [n_mats, 20] of n_mats x 64 bytes of materials"""
    m = np.ascontiguousarray(materials).view(np.uint8).reshape(-1).view(np.uint32).reshape(-1, MAT_WORDS)
    desc, _ = describe(textures)
    rec = np.zeros((len(m), RECORD_WORDS), dtype=np.uint32)
    rec[:, :MAT_WORDS] = m
    dtex = m[:, 0].view(np.int32)
    has = (dtex >= 0) & (dtex < len(textures))
    if has.any():
        rec[has, MAT_WORDS:] = desc[dtex[has]].view(np.uint32)
    return rec


def pack(materials, textures):
    """(records, arena, descriptors): what api.pack_appearance gives"""
    return records(materials, textures), arena(textures), describe(textures)[0]
