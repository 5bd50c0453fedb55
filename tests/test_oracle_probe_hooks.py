"""CPU tests of the oracle's per-piece hooks that the device probes (tests/test_gpu_device_probes.py) compare against and that no other CPU
test reaches: orc_normalize3 and orc_sample_texture, each against an independent binary64 evaluation."""
import numpy as np

from oracle import oracle_py as O

F64 = np.float64


def test_oracle_abi_version():
    assert O.lib().orc_abi_version() == 3


def test_normalize3_against_fp64():
    rs = np.random.RandomState(1)
    v = (rs.normal(size=(20000, 3)) * 2.0 ** rs.randint(-55, 55, size=(20000, 1))).astype(np.float32)
    out = O.normalize3(v)
    want = v.astype(F64) / np.linalg.norm(v.astype(F64), axis=1, keepdims=True)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(F64)
    assert (np.abs(out - want) <= 4 * ulp).all()
    assert np.abs(np.linalg.norm(out.astype(F64), axis=1) - 1).max() < 3e-7
    # the canonical formula v * (1 / sqrt(dot)) at its edges: 0 * inf, a squared length that underflows or overflows
    edge = O.normalize3(np.float32([[0, 0, 0], [1e-30, 0, 0], [2.0 ** 127, 0, 0], [3, 0, -4], [0, -2, 0]]))
    assert np.isnan(edge[0]).all() and np.isinf(edge[1, 0]) and np.isnan(edge[1, 1]) and not edge[2].any()
    assert np.array_equal(edge[3], np.float32([3, 0, -4]) * (np.float32(1) / np.float32(5))) and np.array_equal(edge[4], np.float32([0, -1, 0]))


def _bilinear_fp64(rgb, s, t):
    """GL_LINEAR / GL_REPEAT in binary64, written from the GL specification's formula"""
    h, w, _ = rgb.shape
    u, v = s.astype(F64) * w - 0.5, t.astype(F64) * h - 0.5
    i0, j0 = np.floor(u), np.floor(v)
    a, b = (u - i0)[:, None], (v - j0)[:, None]
    i0, j0 = i0.astype(np.int64) % w, j0.astype(np.int64) % h
    i1, j1 = (i0 + 1) % w, (j0 + 1) % h
    c = rgb.astype(F64) / 255.0
    return (1 - a) * (1 - b) * c[j0, i0] + a * (1 - b) * c[j0, i1] + (1 - a) * b * c[j1, i0] + a * b * c[j1, i1]


def test_sample_texture_against_fp64_bilinear():
    rs = np.random.RandomState(2)
    for w, h in ((1, 1), (3, 5), (64, 64), (257, 2)):
        rgb = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        s, t = rs.uniform(-3, 3, size=5000).astype(np.float32), rs.uniform(-3, 3, size=5000).astype(np.float32)
        out = O.sample_texture(rgb, s, t)
        assert np.abs(out - _bilinear_fp64(rgb, s, t)).max() < 2e-4 * max(w, h)   # the weights come from s * w - 0.5 in binary32 near |s w| = 3 w
        # at a texel centre the fetch is the texel itself, c / 255 rounded once, and the texture repeats with period 1
        ii, jj = rs.randint(0, w, size=500), rs.randint(0, h, size=500)
        ii[:50], jj[:50] = w // 2, h // 2                                         # ((w // 2) + 0.5) / w is a binary32 for every w here
        for shift in (0.0, 1.0, -2.0):
            sc = ((ii + 0.5) / w + shift).astype(np.float32)
            tc = ((jj + 0.5) / h + shift).astype(np.float32)
            exact = (np.floor(sc.astype(F64) * w - 0.5) == sc.astype(F64) * w - 0.5) & (np.floor(tc.astype(F64) * h - 0.5) == tc.astype(F64) * h - 0.5)
            assert exact.sum() >= 50
            got = O.sample_texture(rgb, sc, tc)[exact]
            assert np.array_equal(got, rgb[jj, ii][exact].astype(np.float32) / np.float32(255))
    # a constant texture: the four weights sum to 1 up to rounding; absurd coordinates stay finite, infinite ones give NaN weights
    flat = np.full((4, 4, 3), 200, np.uint8)
    far = O.sample_texture(flat, np.float32([0.3, -7.7, 1e9, -3e9, 123456.7]), np.float32([0.9, 2.2, -1e9, 3e9, -0.0]))
    assert np.abs(far - 200 / 255.0).max() < 2e-7
    assert np.isnan(O.sample_texture(flat, np.float32([np.inf]), np.float32([0.5]))).all()
