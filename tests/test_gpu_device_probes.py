"""-m gpu: the device helpers of csrc/device (canon_math.hpp, shade.hpp, noise.hpp) ONE BY ONE, through adypt_amd/libadypt_probe.so
(tests/probe.py), against the oracle's piece of the same name and — wherever one exists — against a truth that needs neither side: IEEE
division, integer shifts, numpy's float32, exact rational arithmetic.  The render and ray-batch tests hold these helpers only at the inputs a
few scenes produce; here the inputs are dense sweeps and the edges (zeros, denormals, infinities, NaN, exponent 253+, bytes 0 and 255,
partial EXEC, grazing incidence, ior 0 / inf).

Comparison: probe.same — equal bits, or NaN on both sides.  Every test asserts, from its inputs or from the truth's side and never from
the device's output, that the branch it exists for is reached.  Two input classes are left out because the CPU side is undefined there:
NaN texture coordinates ((int)NaN) and, for sincos, non-finite x or |x| > 2^40 (the (long long) conversion of the quadrant)."""
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import oracle_py as O  # noqa: E402
from tests import noise_truth as NT  # noqa: E402
from tests import probe as P  # noqa: E402
from tests.probe import same  # noqa: E402

F32, U32, F64 = np.float32, np.uint32, np.float64
INF, NAN = F32(np.inf), F32(np.nan)
ONE = F32(1.0)
BELOW_ONE, ABOVE_ONE = np.nextafter(ONE, F32(0)), np.nextafter(ONE, F32(2))
DENORM_MIN, DENORM_MAX = U32(1).view(F32), U32(0x007fffff).view(F32)


def f32(bits_):
    return np.ascontiguousarray(bits_, dtype=U32).view(F32)


def u32(x):
    return np.ascontiguousarray(x, dtype=F32).view(U32)


def check(got, want, what, *inputs):
    """probe.same everywhere; the message names the first mismatches with their inputs."""
    ok = same(got, want)
    if not ok.all():
        rows = np.unique(np.argwhere(~ok)[:, 0])[:6]
        got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
        lines = ["row %d: in %s device %s (%s) truth %s (%s)" % (r, [np.asarray(a)[r].tolist() for a in inputs], got[r].tolist(),
                 np.vectorize(hex)(got.view(U32)[r]).tolist(), want[r].tolist(), np.vectorize(hex)(want.view(U32)[r]).tolist()) for r in rows]
        raise AssertionError("%s: %d of %d values differ\n%s" % (what, int((~ok).sum()), ok.size, "\n".join(lines)))


def is_denormal(x):
    x = np.asarray(x, F32)
    return (x != 0) & (np.abs(x) < F32(2.0 ** -126))


def report(name, **figures):
    print("probe %-18s %s" % (name, "  ".join("%s=%s" % kv for kv in figures.items())))


def edge_pairs():
    """all pairs of: +-0, +-denormal, +-1, the floats next to 1, +-inf, NaN"""
    v = F32([0.0, -0.0, DENORM_MIN, -DENORM_MIN, DENORM_MAX, 1.0, -1.0, BELOW_ONE, ABOVE_ONE, -BELOW_ONE, np.inf, -np.inf, np.nan])
    a, b = np.meshgrid(v, v, indexing="ij")
    return a.reshape(-1).copy(), b.reshape(-1).copy()


# ------------------------------------------------------------------------------------------------------------------------------
# canon_math.hpp
# ------------------------------------------------------------------------------------------------------------------------------
def _ieee_reciprocal(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = ONE / x
    assert r.dtype == F32
    return r


def _division_branch(x):
    """rcp_ieee's second branch: biased exponent 0, 253, 254, 255"""
    e = (u32(x) >> 23) & 0xff
    return (e == 0) | (e >= 253)


def test_rcp_every_exponent_and_the_specials():
    rs = np.random.RandomState(1)
    mant = np.concatenate([[0, 1, 0x400000, 0x7fffff], rs.randint(0, 1 << 23, size=60)]).astype(U32)
    sign, expo = U32([0, 0x80000000]), np.arange(256, dtype=U32)
    grid = (sign[:, None, None] | (expo[None, :, None] << 23) | mant[None, None, :]).reshape(-1)
    x = np.concatenate([f32(grid), F32([0.0, -0.0, np.inf, -np.inf, np.nan])])
    e = (u32(x) >> 23) & 0xff
    assert set(range(256)) == set(np.unique(e).tolist())                      # exponents 0, 253, 254, 255 among them
    assert min(int((e == k).sum()) for k in (0, 253, 254, 255)) >= 128 and np.isnan(x).sum() > 100 and is_denormal(x).sum() >= 126
    report("rcp", inputs=len(x), division_branch=int(_division_branch(x).sum()), nan=int(np.isnan(x).sum()))
    check(P.rcp(x), _ieee_reciprocal(x), "rcp_ieee against IEEE 1 / x", x)


def test_rcp_sweep_of_2_to_24_patterns():
    x = f32((np.arange(1 << 24, dtype=U32) << 8) | U32(0x5b))
    e = (u32(x) >> 23) & 0xff
    assert set(range(256)) == set(np.unique(e).tolist()) and int(_division_branch(x).sum()) == 8 * (1 << 15)
    report("rcp sweep", inputs=len(x), division_branch=int(_division_branch(x).sum()))
    check(P.rcp(x), _ieee_reciprocal(x), "rcp_ieee against IEEE 1 / x", x)


def test_normalize():
    rs = np.random.RandomState(2)
    n = 40000
    v = (rs.normal(size=(n, 3)) * 2.0 ** rs.randint(-60, 60, size=(n, 1))).astype(F32)
    length = np.linalg.norm(v.astype(F64), axis=1)
    keep = (length >= 2.0 ** -60) & (length <= 2.0 ** 60)
    v = v[keep]
    assert len(v) > 0.95 * n
    got = P.normalize(v)
    check(got, O.normalize3(v), "normalize3 against the oracle", v)
    # independently: within 4 ulp (binary32) of the binary64 value
    want = v.astype(F64) / np.linalg.norm(v.astype(F64), axis=1, keepdims=True)
    ulp = np.spacing(np.abs(want).astype(F32)).astype(F64)
    assert (np.abs(got.astype(F64) - want) <= 4 * ulp).all(), "normalize3: %g ulp from v / |v|" % (np.abs(got - want) / ulp).max()
    # zero, denormal and 2^127 vectors: NaN, inf and 0 results as the oracle's
    big = F32(2.0 ** 127)
    edge = np.array([[0, 0, 0], [-0.0, 0, 0], [DENORM_MIN, 0, 0], [DENORM_MAX, DENORM_MAX, DENORM_MAX], [0, -DENORM_MAX, DENORM_MIN],
                     [F32(2.0 ** -75), 0, 0], [F32(2.0 ** -74), F32(2.0 ** -75), 0], [F32(1e-30), F32(-1e-30), DENORM_MAX],
                     [big, 0, 0], [big, big, -big], [0, -big, 1], [F32(2.0 ** 64), F32(2.0 ** 63), 0], [F32(3e38), F32(1e-38), 1],
                     [np.inf, 1, 1], [np.nan, 1, 1], [1, 0, 0], [0, -1, 0]], F32)
    truth = O.normalize3(edge)
    n_nan, n_inf, n_zero = int(np.isnan(truth).any(1).sum()), int(np.isinf(truth).any(1).sum()), int((truth == 0).all(1).sum())
    assert n_nan >= 3 and n_inf >= 1 and n_zero >= 2, (n_nan, n_inf, n_zero)
    report("normalize", inputs=len(v) + len(edge), nan_rows=n_nan, inf_rows=n_inf, zero_rows=n_zero)
    check(P.normalize(edge), truth, "normalize3 at the edges against the oracle", edge)


def _quadrants(x):
    return np.unique(np.rint(x.astype(F64) * 0.63661977236758134308).astype(np.int64) & 3).tolist()


def _check_sincos(x, what):
    assert np.isfinite(x).all() and np.abs(x).max() <= 2.0 ** 40      # beyond: the (long long) conversion is undefined on the CPU
    ts, tc = O.sincos(x)
    assert np.isfinite(ts).all() and np.isfinite(tc).all()
    gs, gc = P.sincos(x)
    check(gs, ts, "canon_sincos, sine, " + what, x)
    check(gc, tc, "canon_sincos, cosine, " + what, x)


def test_sincos_the_shader_domain():
    """every phi the shader can form: rx * 6.28318530718f for the 2^24 values k / 2^24 of a Sobol coordinate"""
    x = (np.arange(1 << 24, dtype=F64) / 2.0 ** 24).astype(F32) * F32(6.28318530718)
    assert x.dtype == F32 and _quadrants(x) == [0, 1, 2, 3]
    report("sincos domain", inputs=len(x))
    _check_sincos(x, "shader domain")


def test_sincos_beyond_the_domain_and_tiny():
    lin = np.linspace(0.0, 100.0, 50001).astype(F32)
    big = F32([2.0 ** 20, 2.0 ** 31, 2.0 ** 40, np.nextafter(F32(2.0 ** 31), F32(0)), np.nextafter(F32(2.0 ** 40), F32(0))])
    den = np.concatenate([f32(np.random.RandomState(3).randint(1, 1 << 23, size=500)), [DENORM_MIN, DENORM_MAX, F32(2.0 ** -126), F32(1e-30)]]).astype(F32)
    x = np.concatenate([lin, -lin, big, -big, F32([0.0, -0.0]), den, -den])
    assert _quadrants(x) == [0, 1, 2, 3] and is_denormal(x).sum() >= 1000 and (u32(x) == 0x80000000).any()
    report("sincos edges", inputs=len(x), denormal=int(is_denormal(x).sum()), above_2_31=int((np.abs(x) >= 2.0 ** 31).sum()))
    _check_sincos(x, "large and tiny arguments")


def _check_pow(x, y, what):
    x, y = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(y, dtype=F32)
    truth = O.pow_(x, y)
    check(P.pow_(x, y), truth, "canon_pow, " + what, x, y)
    return truth


@pytest.mark.parametrize("e", [0.0, 0.31, 0.5, 2.0, 25.0, 400.0, 1e4])
def test_pow_hemisphere_exponents(e):
    """cos(theta) = pow(1 - r.y, 1 / (e + 1)) over r.y = k / 2^20"""
    x = ONE - (np.arange(1 << 20, dtype=F64) / 2.0 ** 20).astype(F32)
    y = np.full(len(x), ONE / (F32(e) + ONE), F32)
    assert x.dtype == F32 and x.min() > 0 and x.max() == 1
    truth = _check_pow(x, y, "hemisphere e = %g" % e)
    assert (truth > 0).all() and (truth <= 1).all()
    report("pow hemisphere", e=e, inputs=len(x))


def test_pow_glossy_lobe_underflows_through_the_denormals():
    grid = np.linspace(0.0, 1.0, 20001).astype(F32)
    extra = np.concatenate([[BELOW_ONE, ABOVE_ONE, -0.0, -1e-3, -0.5, -1.0, DENORM_MIN, DENORM_MAX, F32(2.0 ** -126)],
                            f32(np.random.RandomState(4).randint(1, 1 << 23, size=200))]).astype(F32)
    x = np.concatenate([grid, extra])
    figures = {}
    for y in (0.31, 2.0, 100.0, 1e3, 1e4):
        truth = _check_pow(x, np.full(len(x), y, F32), "lobe exponent %g" % y)
        figures[y] = (int(is_denormal(truth).sum()), int((truth == 0).sum()))
    # the final (float)(q * scale) rounds into the denormals or to zero: both must be there, on the oracle's side (measured: 1279 and 7072 on the grid)
    t100 = O.pow_(grid, np.full(len(grid), 100.0, F32))
    assert is_denormal(t100).sum() >= 30 and (t100 == 0).sum() >= 1000, (is_denormal(t100).sum(), (t100 == 0).sum())
    report("pow lobe", inputs=5 * len(x), denormal_and_zero_results_by_exponent=figures)


def test_pow_gamma_curve():
    x = np.concatenate([np.linspace(0.0, 4.0, 400001), [np.inf, np.nan, -1.0, -0.0, DENORM_MIN, DENORM_MAX, 1.0, BELOW_ONE, ABOVE_ONE]]).astype(F32)
    y = np.full(len(x), ONE / F32(2.2), F32)
    truth = _check_pow(x, y, "gamma 1 / 2.2")
    assert np.isnan(truth).sum() >= 2 and np.isinf(truth).sum() == 1                 # NaN in and negative x; +inf stays +inf
    report("pow gamma", inputs=len(x))


def test_pow_special_case_ladder():
    v = F32([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, 1e-38, 3.4e38, 0.5, 2.0, BELOW_ONE, ABOVE_ONE])
    x, y = [a.reshape(-1) for a in np.meshgrid(v, v, indexing="ij")]
    truth = _check_pow(x, y, "special cases")
    # every rung of the ladder, counted on the oracle's side / the inputs
    assert ((y == 0) & (truth == 1)).sum() == 2 * len(v)                                 # y = +-0 -> 1, NaN base included
    assert np.isnan(truth).sum() >= 2 * len(v) - 2 and ((x < 0) & (y != 0) & ~np.isnan(y)).sum() >= 20
    assert ((x == 0) & (y < 0) & np.isinf(truth)).sum() == 4 and ((x == np.inf) & (y < 0) & (truth == 0)).sum() == 2  # (+-0, +inf) ^ (-1, -inf)
    assert ((y == 1) & (x > 0) & np.isfinite(x)).sum() >= 7 and np.isinf(truth).sum() >= 20 and (truth == 0).sum() >= 20
    report("pow specials", inputs=len(x), nan=int(np.isnan(truth).sum()), inf=int(np.isinf(truth).sum()), zero=int((truth == 0).sum()))


def test_unorm8_masks_the_low_byte():
    byte = np.arange(256, dtype=U32)
    rs = np.random.RandomState(5)
    garbage = [np.full(256, 0xffffff, U32), np.full(256, 0xaaaaaa, U32), rs.randint(1, 1 << 24, size=256).astype(U32)]
    c = np.concatenate([byte | (g << 8) for g in garbage] + [byte])                    # three kinds of upper 24 bits, then the plain bytes
    want = (c & 0xff).astype(F32) / F32(255.0)
    assert want.dtype == F32 and (c >> 8 != 0).sum() == 768 and len(np.unique(c[:768] >> 8)) > 200
    report("unorm8", inputs=len(c))
    check(P.unorm8(c), want, "unorm8_to_float against c / 255", c)


def test_exp_byte_and_shl_bytes_every_byte_value():
    rs = np.random.RandomState(6)
    # exp_byte: every value in every byte position, the other bytes random
    words = []
    for pos in range(4):
        w = rs.randint(0, 1 << 32, size=(4, 256), dtype=np.uint64).astype(U32)
        w = (w & ~U32(0xff << (8 * pos))) | (np.arange(256, dtype=U32) << (8 * pos))
        words.append(w.reshape(-1))
    w = np.concatenate(words)
    want = np.stack([((w >> (8 * j)) & 0xff) << 23 for j in range(3)], 1).astype(U32)
    got = P.exp_byte(w)
    assert np.array_equal(got, want), "exp_byte: rows %s" % np.unique(np.argwhere(got != want)[:, 0])[:8]
    for j in range(3):
        assert set(((w >> (8 * j)) & 0xff).tolist()) == set(range(256))
    # shl_bytes: every (shift byte, value byte) pair in every position, the other bytes random
    sb, xb = [a.reshape(-1).astype(U32) for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij")]
    s_all, x_all = [], []
    for pos in range(4):
        keep = ~U32(0xff << (8 * pos))
        s_all.append((rs.randint(0, 1 << 32, size=len(sb), dtype=np.uint64).astype(U32) & keep) | (sb << (8 * pos)))
        x_all.append((rs.randint(0, 1 << 32, size=len(sb), dtype=np.uint64).astype(U32) & keep) | (xb << (8 * pos)))
    s, x = np.concatenate(s_all), np.concatenate(x_all)
    want = np.stack([((((x >> (8 * j)) & 0xff).astype(np.uint64) << (((s >> (8 * j)) & 0xff) & 31).astype(np.uint64)) & 0xffffffff).astype(U32)
                     for j in range(4)], 1)
    got = P.shl_bytes(s, x)
    assert np.array_equal(got, want), "shl_bytes: rows %s" % np.unique(np.argwhere(got != want)[:, 0])[:8]
    report("exp_byte/shl_bytes", exp_byte_inputs=len(w), shl_bytes_inputs=len(s))


LANE_MASKS = {"all lanes": (1 << 64) - 1, "odd lanes": 0xaaaaaaaaaaaaaaaa, "one lane": 1 << 17, "no lane": 0, "upper 32": 0xffffffff00000000}


@pytest.mark.parametrize("which", list(LANE_MASKS))
def test_or_if_le_under_partial_exec(which):
    mask = LANE_MASKS[which]
    a, b = edge_pairs()
    n_pairs = len(a)
    assert n_pairs % 2 == 1                                           # coprime with 64: over 64 repetitions every pair meets every lane
    a, b = np.tile(a, 64)[:-37], np.tile(b, 64)[:-37]                 # (the last wave is a partial one)
    n = len(a)
    rs = np.random.RandomState(7)
    A = rs.randint(0, 1 << 16, size=n).astype(U32)                    # three disjoint bit ranges: what came from where is visible
    bits_ = (rs.randint(1, 1 << 15, size=n).astype(U32)) << 16
    B = np.full(n, 0x80000000, U32)
    selected = np.array([(mask >> lane) & 1 for lane in range(64)], bool)[np.arange(n) & 63]
    with np.errstate(invalid="ignore"):
        le = a <= b                                                   # IEEE: false with a NaN, true for (+0, -0) and (-0, +0)
    want = A | np.where(selected & le, bits_, U32(0)) | B
    if 0 < mask < (1 << 64) - 1:
        pair = np.arange(n) % n_pairs
        assert len(np.unique(pair[selected & le])) == le[:n_pairs].sum() and len(np.unique(pair[~selected])) == n_pairs
    assert le[:n_pairs].sum() > 60 and (~le[:n_pairs]).sum() > 60 and np.isnan(a).sum() > 0
    got = P.or_if_le(A, a, b, bits_, B, mask)
    assert (got & B == B).all(), "%s: EXEC was not restored — the OR after the branch missed lanes %s" % (which, np.nonzero(got & B != B)[0][:8])
    assert np.array_equal(got[~selected], (A | B)[~selected]), "%s: lanes outside the mask were touched" % which
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: elements %s: a %s b %s" % (which, bad[:8], a[bad[:8]], b[bad[:8]])
    report("or_if_le", mask=which, inputs=n, selected=int(selected.sum()), selected_and_le=int((selected & le).sum()))


def test_minmax_at_nan_and_signed_zeros():
    a, b = edge_pairs()
    got = P.minmax(a, b)
    with np.errstate(invalid="ignore"):
        zeros = (a == 0) & (b == 0) & (u32(a) != u32(b))              # (+0, -0) and (-0, +0): IEEE maxNum / minNum may return either
        assert zeros.sum() == 2
        for col, name, truth in ((0, "max_num", np.fmax(a, b)), (1, "min_num", np.fmin(a, b))):
            ok = same(got[:, col], truth) | (zeros & (got[:, col] == 0))
            assert ok.all(), "%s: pairs %s" % (name, [(a[i], b[i], got[i, col]) for i in np.nonzero(~ok)[0][:8]])
        check(got[:, 2], np.where(b < a, b, a), "gl_min", a, b)       # y < x ? y : x
        check(got[:, 3], np.where(a < b, b, a), "gl_max", a, b)       # x < y ? y : x
    n_nan = int((np.isnan(a) | np.isnan(b)).sum())
    assert n_nan == 25
    report("minmax", inputs=len(a), pairs_with_nan=n_nan, signed_zero_pairs=2)


def _round_to_f32(fr):
    """the binary32 nearest to the rational fr, ties to even, denormals and overflow included (fr != 0)"""
    sign = -1.0 if fr < 0 else 1.0
    fr = abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    assert Fraction(2) ** e <= fr < Fraction(2) ** (e + 1)
    e = max(e, -126)
    q = fr / Fraction(2) ** (e - 23)
    m = q.numerator // q.denominator
    rem = q - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    v = Fraction(m) * Fraction(2) ** (e - 23)
    return F32(sign * (np.inf if v >= Fraction(2) ** 128 else float(v)))


def test_pk_fma_hi_is_one_ieee_fma_per_half():
    rs = np.random.RandomState(8)
    n = 4096

    def rnd(lo, hi, shape):
        return ((1.0 + rs.uniform(size=shape)) * 2.0 ** rs.randint(lo, hi, size=shape) * rs.choice([-1.0, 1.0], size=shape)).astype(F32)

    a, b, c = rnd(-8, 8, (n, 2)), rnd(-8, 8, (n, 2)), rnd(-8, 8, (n, 2))
    k = n // 4
    # cancellation: c = -(a * b.y rounded), the fma returns the rounding error of the product (exactly zero where there is none)
    for v in (a, b):                                                  # (8-bit significands: these products are exact)
        v[:64] = (rs.randint(128, 256, size=(64, 2)) * 2.0 ** rs.randint(-8, 8, size=(64, 2)) * rs.choice([-1.0, 1.0], size=(64, 2))).astype(F32)
    c[:k] = -(a[:k] * b[:k, 1:2])
    # large exponents: overflow to inf, results in and below the denormals
    a[k:2 * k], b[k:2 * k], c[k:2 * k] = rnd(58, 64, (k, 2)), rnd(60, 66, (k, 2)), rnd(100, 127, (k, 2))
    a[2 * k:3 * k], b[2 * k:3 * k], c[2 * k:3 * k] = rnd(-70, -60, (k, 2)), rnd(-75, -62, (k, 2)), rnd(-149, -126, (k, 2))
    c[2 * k:2 * k + 64] = np.copysign(DENORM_MIN, c[2 * k:2 * k + 64])                  # the product lies far below the least denormal: it only decides the rounding
    want = np.empty((n, 2), F32)
    for i in range(n):
        for h in range(2):
            exact = Fraction(float(a[i, h])) * Fraction(float(b[i, 1])) + Fraction(float(c[i, h]))
            want[i, h] = F32(0.0) if exact == 0 else _round_to_f32(exact)           # (no zero operands: an exact zero sum is +0)
    assert (a != 0).all() and (b != 0).all() and (c != 0).all()
    n_zero, n_inf, n_den = int((want == 0).sum()), int(np.isinf(want).sum()), int(is_denormal(want).sum())
    assert n_zero >= 20 and n_inf >= 50 and n_den >= 200 and ((want[:k] != 0) & (np.abs(want[:k]) < 1e-4 * np.abs(c[:k]))).sum() >= 500
    hi, plain = P.pk_fma_hi(a, b, c)
    check(hi, plain, "pk_fma_hi against pk_fma(a, v2s(b.y), c) on the device", a, b, c)
    check(hi, want, "pk_fma_hi against the exact result rounded once", a, b, c)
    check(plain, want, "pk_fma against the exact result rounded once", a, b, c)
    report("pk_fma_hi", inputs=n, zero=n_zero, inf=n_inf, denormal=n_den)


# ------------------------------------------------------------------------------------------------------------------------------
# shade.hpp
# ------------------------------------------------------------------------------------------------------------------------------
def test_sobol2_wraps_at_one():
    rs = np.random.RandomState(9)
    n = 20000
    q, s = rs.uniform(size=(n, 2)).astype(F32), rs.uniform(size=(n, 2)).astype(F32)
    # sums one and two ulp either side of 1, and 1 itself
    targets = F32([np.nextafter(BELOW_ONE, F32(0)), BELOW_ONE, ONE, ABOVE_ONE, np.nextafter(ABOVE_ONE, F32(2))])
    qe = rs.uniform(0.25, 0.75, size=(2000, 2)).astype(F32)
    se = (targets[rs.randint(0, 5, size=(2000, 2))] - qe).astype(F32)
    q, s = np.concatenate([q, qe, F32([[0, 0], [0, BELOW_ONE], [BELOW_ONE, BELOW_ONE], [0.5, 0.5]])]), \
        np.concatenate([s, se, F32([[0, 0], [BELOW_ONE, 0], [BELOW_ONE, BELOW_ONE], [0.5, 0.5]])])
    q[q >= 1], s[s >= 1] = BELOW_ONE, BELOW_ONE
    assert (q >= 0).all() and (q < 1).all() and (s >= 0).all() and (s < 1).all()
    a = q + s
    want = a - np.floor(a)
    assert a.dtype == F32 and want.dtype == F32
    for t in targets:
        assert (a == t).sum() >= 50, (t, (a == t).sum())
    assert (a >= 1).sum() > 5000 and (a < 1).sum() > 5000 and (want >= 0).all() and (want < 1).all()
    via_rng, via_point = P.sobol2(q, s)
    check(via_rng, want, "sobol2(Rng)", q, s)
    check(via_point, want, "sobol2(RngPoint)", q, s)
    report("sobol2", inputs=len(q), sums_at_or_next_to_one=int(np.isin(a, targets).sum()))


@pytest.mark.parametrize("e", [0.0, 0.5, 2.0, 25.0, 400.0])
def test_sample_hemisphere_stratified_grid(e):
    k = 384
    g = (np.arange(k) + 0.5) / k                                      # the grid of tests/test_oracle_shading.py::test_sample_hemisphere_moments
    r = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2).astype(F32)
    check(P.sample_hemisphere(r, e), O.sample_hemisphere(r, e), "sample_hemisphere e = %g" % e, r)
    report("sample_hemisphere", e=e, inputs=len(r))


@pytest.mark.parametrize("e", [0.31, 1e4, 1e30])
def test_sample_hemisphere_at_the_ends_of_the_unit_interval(e):
    v = F32([0.0, BELOW_ONE, 1.0, 0.25, 0.5])
    r = np.stack(np.meshgrid(v, v, indexing="ij"), -1).reshape(-1, 2)
    truth = O.sample_hemisphere(r, e)
    # r.y = 1 wraps to 0 in Sobol(): the pole, like r.y = 0; the float below 1 is the lowest sample of the lobe
    assert (truth[r[:, 1] == 0][:, 2] == 1).all() and np.array_equal(u32(truth[r[:, 1] == 1]), u32(truth[r[:, 1] == 0]))
    assert (truth[r[:, 1] == BELOW_ONE][:, 2] < 1).all() == (e < 1e30)
    check(P.sample_hemisphere(r, e), truth, "sample_hemisphere e = %g" % e, r)
    report("sample_hemisphere ends", e=e, inputs=len(r))


def _units(rs, n):
    v = rs.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def test_align_direction():
    rs = np.random.RandomState(10)
    n = 20000
    d, t = _units(rs, n), _units(rs, n)
    # target.x at the threshold 0.01f, its neighbours, both signs
    thr = F32(0.01)
    xs = F32([thr, np.nextafter(thr, F32(0)), np.nextafter(thr, F32(1)), -thr, -np.nextafter(thr, F32(0)), -np.nextafter(thr, F32(1)), 0.0, -0.0])
    t_thr = _units(rs, 800)
    t_thr[:, 0] = np.tile(xs, 100)
    axes = F32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    odd = F32([[0, 0, 0], [-0.0, 0, 0], [0, 0, 0]])                   # cross(a, 0) = 0, normalize(0) = NaN on both sides
    scaled = (_units(rs, 500) * (2.0 ** rs.randint(-40, 40, size=(500, 1)))).astype(F32)
    t = np.concatenate([t, t_thr, axes, odd, scaled])
    d = np.concatenate([d, _units(rs, len(t) - n)])
    truth = O.align_direction(d, t)
    wide = np.abs(t[:, 0]) > thr
    assert wide.sum() > 10000 and (~wide).sum() > 500 and (np.abs(t_thr[:, 0]) > thr).sum() == 200 and (np.abs(t_thr[:, 0]) == thr).sum() == 200
    n_nan = int(np.isnan(truth).any(1).sum())
    assert n_nan >= 3
    check(P.align_direction(d, t), truth, "align_direction", d, t)
    report("align_direction", inputs=len(t), helper_axis_y=int(wide.sum()), helper_axis_x=int((~wide).sum()), nan_rows=n_nan)


def _mats(n, illum, kd=(0.5, 0.5, 0.5), ks=(0.5, 0.5, 0.5), shininess=1.0, ior=1.5):
    m = np.zeros(n, dtype=O.MAT_DT)
    m["dtex"] = m["etex"] = m["stex"] = -1
    m["kd"], m["ks"], m["illum"], m["shininess"], m["ior"], m["dissolve"] = kd, ks, illum, shininess, ior, 1.0
    return m


def _respond_inputs():
    """(materials, normal, dir, r) — the inputs of tests/test_oracle_shading.py, then the edges"""
    parts = []

    def add(m, nrm, d, r):
        parts.append((m, np.asarray(nrm, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3), np.asarray(r, F32).reshape(-1, 2)))

    rs = np.random.RandomState(1)
    n = 20000
    add(_mats(n, 3, ks=(0.9, 0.8, 0.7)), _units(rs, n), _units(rs, n), rs.uniform(size=(n, 2)))
    rs = np.random.RandomState(2)
    n = 40000
    nrm, d = _units(rs, n), _units(rs, n)
    m = _mats(n, 7)
    m["ior"] = rs.choice([1.0, 1.33, 1.5, 2.4], size=n).astype(F32)
    m["illum"][::2] = 6
    add(m, nrm, d, rs.uniform(size=(n, 2)))
    rs = np.random.RandomState(3)
    for illum in (0, 8, 9, 11, -3):
        add(_mats(64, illum), _units(rs, 64), _units(rs, 64), rs.uniform(size=(64, 2)))
    rs = np.random.RandomState(4)
    n = 30000
    nrm, d, r = _units(rs, n), _units(rs, n), rs.uniform(size=(n, 2))
    add(_mats(n, 1, kd=(0.2, 0.4, 0.6)), nrm, d, r)
    add(_mats(n, 2, kd=(0.2, 0.4, 0.6), shininess=30.0), nrm, d, r)
    add(_mats(n, 2, kd=(0.3, 0.3, 0.1), ks=(0.5, 0.4, 0.3), shininess=200.0), nrm, d, r)
    # ---- edges ----
    rs = np.random.RandomState(11)
    z = F32([0, 0, 1])
    graze = F32([[1, 0, 0], [1, 0, 1e-30], [1, 0, -1e-30], [0, 1, 0], [0.6, 0.8, 0], [0.6, 0.8, 1e-30], [0, 0, 1], [0, 0, -1],
                 [1, 0, DENORM_MIN], [1, 0, -DENORM_MIN]])            # dir perpendicular to the normal exactly and nearly; dir = +-normal
    iors = F32([0.0, 0.5, 1.0, np.inf, 1.33, 1.5, 2.4])
    rx = F32([0.0, 0.04, 0.5, BELOW_ONE])
    for illum in (1, 2, 3, 6, 7):
        for ior in iors if illum >= 6 else iors[:1]:
            g, x = np.repeat(graze, len(rx), 0), np.tile(rx, len(graze))
            add(_mats(len(g), illum, shininess=200.0, ior=ior), np.tile(z, (len(g), 1)), g, np.stack([x, x], 1))
    # ior edges at every angle, both sides of the surface
    n = 4000
    m = _mats(n, 7)
    m["ior"] = rs.choice(F32([0.0, 0.5, 1.0, np.inf]), size=n)
    m["illum"][::2] = 6
    add(m, _units(rs, n), _units(rs, n), rs.uniform(size=(n, 2)))
    # the glossy threshold: 30 * 0.01f = 0.29999998 stays diffuse, the next float up is glossy
    for ns in (29.999998, 30.0, 30.000002, 31.0, 1e6, -5.0, np.inf):
        n = 1000
        add(_mats(n, 2, kd=(0.3, 0.3, 0.1), ks=(0.5, 0.4, 0.3), shininess=ns), _units(rs, n), _units(rs, n), rs.uniform(size=(n, 2)))
    # non-unit normals, every illum
    n = 700
    m = _mats(n, 1, shininess=200.0)
    m["illum"] = np.tile([1, 2, 3, 5, 6, 7, 9], n // 7)
    add(m, (_units(rs, n) * rs.choice([0.25, 0.999, 1.001, 3.0], size=(n, 1))).astype(F32), _units(rs, n), rs.uniform(size=(n, 2)))
    m, nrm, d, r = [np.concatenate(x) for x in zip(*parts)]
    # the Fresnel coin at its edge: r.x = the oracle's Fresnel value and its two neighbours (the value does not depend on r)
    glass = np.nonzero((m["illum"] >= 6) & (m["illum"] <= 7))[0][:6000]
    fres = O.scatter(m[glass], nrm[glass], d[glass], r[glass])[:, 6]
    fin = glass[np.isfinite(fres)]
    fres = fres[np.isfinite(fres)]
    edge_r = np.concatenate([np.stack([x, np.full(len(x), 0.5, F32)], 1) for x in (fres, np.nextafter(fres, -INF), np.nextafter(fres, INF))])
    three = np.concatenate([fin, fin, fin])
    return np.concatenate([m, m[three]]), np.concatenate([nrm, nrm[three]]), np.concatenate([d, d[three]]), np.concatenate([r, edge_r]), len(fin)


def test_respond_against_the_oracle_scatter():
    m, nrm, d, r, n_coin = _respond_inputs()
    truth = O.scatter(m, nrm, d, r)
    # every branch has members — decided on the oracle's side and from the inputs
    glass = (m["illum"] == 6) | (m["illum"] == 7)
    N, D = nrm.astype(F64), d.astype(F64)
    cosi = np.sum(D * N, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        eta = np.where(cosi > 0, m["ior"].astype(F64), 1.0 / m["ior"].astype(F64))
        sint = eta * np.sqrt(np.maximum(0.0, 1.0 - cosi * cosi))
        tir = glass & (sint >= 1.001)
        clear = glass & (sint < 0.98) & np.isfinite(truth[:, 6]) & (np.abs(r[:, 0] - truth[:, 6]) > 1e-4)
        refract, reflect = clear & (r[:, 0] >= truth[:, 6]), clear & (r[:, 0] < truth[:, 6])
    assert (truth[tir, 6] == 1).all()
    glossy = (m["illum"] == 2) & (m["shininess"] * F32(0.01) > F32(0.3))
    dead = truth[:, 7] == 0
    nan_rows = np.isnan(truth[:, :6]).any(1)                       # (Ns inf: the lobe's direction is NaN)
    nan_coin = np.isnan(truth[:, 6])                                 # ior 0 / inf: 0 / 0 and inf - inf in the Fresnel term; `sx >= NaN` then reflects
    odd_ior = glass & ((m["ior"] == 0) | np.isinf(m["ior"]))
    counts = dict(inputs=len(m), total_internal_reflection=int(tir.sum()), refract=int(refract.sum()), reflect=int(reflect.sum()),
                  glossy=int(glossy.sum()), dead_glossy=int((dead & glossy).sum()), nan_rows=int(nan_rows.sum()),
                  nan_fresnel_ior_0_or_inf=int((nan_coin & odd_ior).sum()), nan_rows_ns_inf=int((nan_rows & np.isinf(m["shininess"])).sum()),
                  fresnel_coin_edges=3 * n_coin)
    report("respond", **counts)
    assert tir.sum() > 1000 and refract.sum() > 5000 and reflect.sum() > 500 and n_coin > 3000
    assert (dead & glossy).sum() > 1000 and not (dead & ~glossy).any()
    assert (nan_coin & odd_ior).sum() > 100 and (nan_rows & np.isinf(m["shininess"])).sum() > 100 and not nan_coin[~odd_ior].any()
    assert (m["illum"] == 2).sum() - glossy.sum() >= 30000 + 2000                      # Ns 30 and 29.999998 stay diffuse (and -5)
    direction, color, ret, alive = P.respond(m, nrm, d, r, max_bounce=8)
    assert np.array_equal(alive, ~dead), "alive differs in rows %s" % np.nonzero(alive == dead)[0][:8]
    check(direction, truth[:, 0:3], "respond: new direction", m["illum"], m["shininess"], m["ior"], nrm, d, r)
    check(color, truth[:, 3:6], "respond: throughput", m["illum"], m["shininess"], m["ior"], nrm, d, r)
    assert not ret.any()                                                                # no emission anywhere: fma(1, 0, 0)


def test_respond_emission_and_last_bounce():
    """what orc_scatter does not return, asserted directly: ret picks the emission up; at the loop's last iteration nothing else happens"""
    rs = np.random.RandomState(12)
    n = 7 * 300
    m = _mats(n, 1, shininess=200.0)
    m["illum"] = np.tile([1, 2, 3, 5, 6, 7, 9], n // 7)
    ke = rs.uniform(0.0, 8.0, size=(n, 3)).astype(F32)
    ke[:50] = F32([DENORM_MIN, 3e38, 0.0])
    ke[50:100] = F32([np.inf, DENORM_MAX, 1e-30])
    m["ke"] = ke
    nrm, d, r = _units(rs, n), _units(rs, n), rs.uniform(size=(n, 2)).astype(F32)
    truth = O.scatter(m, nrm, d, r)
    direction, color, ret, alive = P.respond(m, nrm, d, r, max_bounce=8)
    assert np.array_equal(u32(ret), u32(ke)), "ret = fma(color 1, Ke, ret 0) must be Ke"
    assert np.array_equal(alive, truth[:, 7] == 1)
    check(direction, truth[:, 0:3], "respond with emission: direction", m["illum"], nrm, d, r)
    check(color, truth[:, 3:6], "respond with emission: throughput", m["illum"], nrm, d, r)
    assert (alive & (u32(direction) != u32(d)).any(1)).sum() > 0.8 * n
    direction, color, ret, alive = P.respond(m, nrm, d, r, max_bounce=1)
    assert not alive.any(), "b + 1 >= max_bounce: the path ends"
    assert np.array_equal(u32(direction), u32(d)) and (color == 1).all(), "the last iteration touched direction or throughput"
    assert np.array_equal(u32(ret), u32(ke))
    report("respond emission", inputs=2 * n)


def _texture_coordinates(w):
    k = np.arange(-2 * w, 2 * w + 1, dtype=F64)
    big = F32(1e9)
    edges = F32([-0.0, 0.0, big, np.nextafter(big, INF), np.nextafter(big, F32(0)), -big, -np.nextafter(big, INF), -np.nextafter(big, F32(0)),
                 3e9, -3e9, np.inf, -np.inf, -1e-7, -0.37, -5.25, 1e-30, -1e-30, 0.999999, 123456.7, -123456.7])
    # coordinates whose texel index floor(s w - 0.5) lands on the clamp at +-1e9 and its neighbours
    clamp = (np.array([1e9, 1e9 + 64, 1e9 - 64, -1e9, -1e9 - 64, -1e9 + 64], F64) / w).astype(F32)
    return np.concatenate([(k / w).astype(F32), ((k + 0.5) / w).astype(F32), edges, clamp])


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (64, 64), (257, 2)])
def test_sample_texture(w, h):
    rs = np.random.RandomState(13)
    rgb = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    rgb.reshape(-1)[:6] = [0, 255, 1, 254, 0, 255][:min(6, rgb.size)]
    s, t = [a.reshape(-1) for a in np.meshgrid(_texture_coordinates(w), _texture_coordinates(h), indexing="ij")]
    assert not np.isnan(s).any() and not np.isnan(t).any()           # (int)NaN is undefined on the CPU: the one excluded input class
    truth = O.sample_texture(rgb, s, t)
    with np.errstate(invalid="ignore", over="ignore"):
        fu = np.floor(s.astype(F64) * w - 0.5)
    n_clamped, n_negative, n_nan = int((np.abs(fu) >= 1e9).sum()), int((fu < 0).sum()), int(np.isnan(truth).any(1).sum())
    assert n_clamped > 0 and n_negative > 0 and n_nan > 0 and np.isfinite(truth).all(1).sum() > 0.5 * len(s)
    check(P.sample_texture(rgb, s, t), truth, "sample_texture %d x %d" % (w, h), s, t)
    report("sample_texture", size="%dx%d" % (w, h), inputs=len(s), clamped=n_clamped, negative_index=n_negative, nan_rows=n_nan)


def _display_inputs():
    k = np.arange(256, dtype=F64)
    edge = (((k + 0.5) / 255.0) ** 2.2).astype(F32)                   # where the gamma curve crosses from byte k to k + 1
    near = [edge]
    lo = hi = edge
    for _ in range(3):
        lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
        near += [lo, hi]
    rs = np.random.RandomState(14)
    vals = np.concatenate(near + [F32([0.0, -0.0, -1.0, -1e-30, np.nan, np.inf, -np.inf, DENORM_MIN, DENORM_MAX, -DENORM_MAX, 1.0, BELOW_ONE, ABOVE_ONE,
                                       2.0, 4.0, 1e30, 3.4e38, 2.0 ** 64, 2.0 ** 127, 1e-30, 0.5, 0.0031308]),
                                  rs.uniform(0.0, 1.2, size=3000).astype(F32), rs.normal(size=3000).astype(F32)])
    vals = np.concatenate([vals, rs.permutation(vals), rs.permutation(vals)])
    vals = vals[:len(vals) // 3 * 3].reshape(-1, 3)
    vectors = np.concatenate([vals, F32([[0, 0, 0], [2.0 ** 127, 2.0 ** 127, 0], [DENORM_MAX, 0, 0], [np.inf, 1, 1], [1, 1, 1], [-1, 0, 0]])])
    return np.concatenate([vectors, rs.uniform(size=(len(vectors), 1)).astype(F32)], 1)


@pytest.mark.parametrize("viewer_type", range(6))
def test_display_kernel(viewer_type):
    rgba = _display_inputs()
    truth = O.display(rgba, viewer_type)
    assert len(np.unique(truth[:, :3])) == 256 and np.isnan(rgba).any() and np.isinf(rgba).any()   # every byte value comes out
    got = P.display(rgba, viewer_type)
    bad = np.nonzero((got != truth).any(1))[0]
    assert len(bad) == 0, "viewer type %d: pixels %s in %s device %s truth %s" % (viewer_type, bad[:6], rgba[bad[:6]], got[bad[:6]], truth[bad[:6]])
    report("display", viewer_type=viewer_type, inputs=len(rgba))


# ------------------------------------------------------------------------------------------------------------------------------
# noise.hpp
# ------------------------------------------------------------------------------------------------------------------------------
def _noise_sequences(k):
    """(elements, k, 3): all zero, constant, one spike among zeros, 1e30 (m2 overflows), denormals, random radiance"""
    rs = np.random.RandomState(15)
    rows = [np.zeros((k, 3)), np.full((k, 3), 0.7), np.full((k, 3), 4.0), np.full((k, 3), 1e30), np.full((k, 3), DENORM_MAX, F64),
            np.full((k, 3), DENORM_MIN, F64), np.full((k, 3), 3e38)]
    for at in sorted({0, k // 2, k - 1}):
        for height in (4.0, 1e30, DENORM_MAX):
            spike = np.zeros((k, 3))
            spike[at] = height
            rows.append(spike)
    alt = np.zeros((k, 3))
    alt[::2] = 1e30
    rows.append(alt)
    rows += [rs.uniform(0, 4, size=(k, 3)) for _ in range(200)]
    rows += [rs.uniform(0, 4, size=(k, 3)) * (rs.uniform(size=(k, 1)) < 0.1) for _ in range(100)]
    rows += [f32(rs.randint(0, 1 << 23, size=(k, 3))).astype(F64) for _ in range(20)]
    return np.array(rows).astype(F32)


@pytest.mark.parametrize("k", [1, 2, 7, 64])
def test_noise_moments_and_estimate(k):
    s = _noise_sequences(k)
    frames = np.ascontiguousarray(s.transpose(1, 0, 2))               # noise_truth.moments: frame-major
    total = 0
    for first, n_frames in [(0, max(k, 2)), (2, 2), (3, 3), (1 << 24, 1 << 24), ((1 << 24) + 1, (1 << 24) + 1)]:
        with np.errstate(all="ignore"):
            mean, m2 = NT.moments(frames, first=first)
            e = NT.noise_e(mean, m2, n_frames)
        if k >= 2:
            assert np.isinf(m2).sum() >= 1 and m2[0] == 0 and e[0] == 0 and np.isfinite(e).sum() > 300
            assert first != 0 or is_denormal(mean).sum() >= 2
        g_mean, g_m2, g_e = P.noise(s, first, n_frames)
        what = "k = %d, first = %d, n = %d" % (k, first, n_frames)
        check(g_mean, mean, "noise_add_sample mean, " + what)
        check(g_m2, m2, "noise_add_sample m2, " + what)
        check(g_e, e, "noise_of_pixel, " + what)
        total += len(s)
    report("noise", k=k, inputs=total)
