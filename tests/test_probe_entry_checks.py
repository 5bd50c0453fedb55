"""CPU test of libadypt_probe.so's entry checks (adypt_amd/csrc/probe/probe.h): a bad element count, size or null pointer is refused before
anything is allocated or launched, so these calls need no GPU.  What the probes compute is tests/test_gpu_device_probes.py's subject."""
import ctypes as C

import numpy as np

from tests import probe as P

INVALID = -1  # -hipErrorInvalidValue
ENTRIES = ("rcp", "normalize", "sincos", "pow", "unorm8", "exp_byte", "shl_bytes", "or_if_le", "minmax", "pk_fma_hi", "sobol2", "sample_hemisphere",
           "align_direction", "respond", "sample_texture", "display", "noise")


def test_every_entry_is_exported():
    for name in ENTRIES:
        assert hasattr(P.lib(), "adypt_probe_" + name), name


def test_bad_counts_sizes_and_null_pointers_are_refused():
    lib = P.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    for n, want in ((-1, INVALID), ((1 << 24) + 1, INVALID), (0, 0)):
        assert lib.adypt_probe_rcp(p, p, C.c_int64(n)) == want
        assert lib.adypt_probe_pow(p, p, p, C.c_int64(n)) == want
        assert lib.adypt_probe_or_if_le(p, p, p, p, p, C.c_uint64(1), p, C.c_int64(n)) == want
        assert lib.adypt_probe_respond(p, p, p, p, C.c_int(8), p, p, p, p, C.c_int64(n)) == want
        assert lib.adypt_probe_display(p, C.c_int(0), p, C.c_int64(n)) == want
    assert lib.adypt_probe_rcp(None, p, C.c_int64(4)) == INVALID and lib.adypt_probe_sincos(p, p, None, C.c_int64(4)) == INVALID
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 24, 2)):
        assert lib.adypt_probe_sample_texture(p, C.c_int(w), C.c_int(h), p, p, p, C.c_int64(4)) == INVALID
    for k, first in ((-1, 0), (4097, 0), (4, -1), (4, 2 ** 31 - 2)):
        assert lib.adypt_probe_noise(p, C.c_int(k), C.c_int(first), C.c_int(2), p, p, p, C.c_int64(4)) == INVALID
    assert lib.adypt_probe_noise(p, C.c_int(4096), C.c_int(0), C.c_int(2), p, p, p, C.c_int64(1 << 13)) == INVALID  # n * k beyond 2^24 samples
