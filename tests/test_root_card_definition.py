"""The root card (csrc/device/root_card.hpp; adypt_decode_root_card): node 0 decoded into the form k_path's shading round tests new rays against,
held against an independent numpy decode of the same 80 bytes — the fields section D of the traversal trip derives per visit.  No GPU."""
import os

import numpy as np
import pytest

from adypt_amd import api
from tests.helpers import GOLDEN, golden_scene


def numpy_card(node, allow=True):
    """The card of one node, from the 80 bytes alone (NodeRec: p[3], e[3], imask, child_base, tri_base, meta[8], qlo x y z [8], qhi x y z [8])."""
    b = np.ascontiguousarray(node, dtype=np.uint8).reshape(80)
    card = np.zeros(1, dtype=api.ROOT_CARD_DT)[0]
    planes = b[32:80].reshape(6, 8)  # qlo x, qlo y, qlo z, qhi x, qhi y, qhi z
    for j in range(8):
        card["q"][j] = [planes[0, j], planes[3, j], planes[1, j], planes[4, j], planes[2, j], planes[5, j]]
    card["scale"] = (b[12:15].astype(np.uint32) << 23).view(np.float32)
    card["origin"] = b[0:12].view(np.float32)
    card["imask"] = b[15]
    card["child_base"], card["tri_base"] = b[16:24].view(np.uint32)
    meta = b[24:32].astype(np.uint32)
    inner = ((meta >> 5) == 1) & ((meta & 31) >= 24) & (meta != 0)  # csrc/device/refit.hpp, the slot kinds
    # section D's bit test for "internal": bits 3 and 4 of meta & 31 both set, i.e. (m & (m << 1)) & 0x10
    inner_d = ((meta & (meta << 1)) & 0x10) != 0
    card["is_inner"] = inner_d
    card["bit_index"] = meta & 31
    card["child_bits"] = (meta >> 5) & 7
    only = bool(np.all((meta == 0) | (inner_d & ((meta >> 5) == 1))))
    card["inner_only"] = only
    card["enabled"] = only and allow
    return card, inner


def synthetic_root(kinds, seed):
    """80 bytes of a root whose slots are of the given kinds: 'i' internal, 'l' leaf (1..3 references), '-' empty."""
    rs = np.random.RandomState(seed)
    b = np.zeros(80, np.uint8)
    b[0:12] = rs.uniform(-3, 3, 3).astype(np.float32).view(np.uint8)
    b[12:15] = rs.randint(110, 135, 3)
    b[16:24] = np.array([1, 0], np.uint32).view(np.uint8)
    imask, n_inner, off = 0, 0, 0
    for j, k in enumerate(kinds):
        if k == "i":
            b[24 + j] = (1 << 5) | (24 + n_inner)
            imask |= 1 << n_inner
            n_inner += 1
        elif k == "l":
            n = 1 + rs.randint(0, 3)
            b[24 + j] = (((1 << n) - 1) << 5) | off
            off += n
        if k != "-":
            lo = rs.randint(0, 200, 3)
            b[32 + j], b[40 + j], b[48 + j] = lo
            b[56 + j], b[64 + j], b[72 + j] = lo + 1 + rs.randint(0, 55, 3)
    b[15] = imask
    return b


def same_card(a, b):
    return a.tobytes() == b.tobytes()


ROOTS = {"all_inner": "iiiiiiii", "one_leaf": "iiiliiii", "three_empty": "ii-i-i-i"}


@pytest.mark.parametrize("name", sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".bvh")))
def test_card_of_a_golden_root_is_the_numpy_decode(name):
    _, _, nodes, _, _, _ = golden_scene(name)
    node = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1, 80)[0]
    want, _ = numpy_card(node)
    assert same_card(api.decode_root_card(node), want)


@pytest.mark.parametrize("kind", sorted(ROOTS))
@pytest.mark.parametrize("allow", [True, False])
def test_card_of_a_synthetic_root_is_the_numpy_decode(kind, allow):
    node = synthetic_root(ROOTS[kind], seed=len(kind))
    want, inner = numpy_card(node, allow)
    got = api.decode_root_card(node, allow)
    assert same_card(got, want)
    # the bit test of the traversal agrees with the builder's definition of an internal slot on these records
    assert np.array_equal(got["is_inner"].astype(bool), inner)
    assert int(got["inner_only"]) == (0 if kind == "one_leaf" else 1)
    assert int(got["enabled"]) == (1 if allow and kind != "one_leaf" else 0)
    if kind == "three_empty":
        assert np.count_nonzero(got["child_bits"]) == 5 and not got["q"][2].any()
