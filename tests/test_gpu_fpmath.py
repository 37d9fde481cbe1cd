"""include/jade_fpmath.h on the device: every routine, run by libjade_hip_debug.so's jade_debug_fpmath (jade_debug_units.hip), must
return the bits the host build of the same header returns (tests/native/fpmath_export.c) - or both a NaN.  tests/test_fpmath.py
pins the host build's accuracy; this file pins "identical to the bit on CPU and GPU", over all exponents, both signs, subnormals,
infinities, NaNs and the branch points of each routine.  sqrt, a / b and 1 / a are compared with numpy float32 too (IEEE, correctly
rounded), which depends neither on the header nor on the host flags: losing -fhip-fp32-correctly-rounded-divide-sqrt or
-fno-gpu-flush-denormals-to-zero fails here."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# jade_debug_units.hip, enum DebugFpOp
(FLOOR, SINCOS, LOG2, EXP2, POW, ATAN, ATAN2, ASIN, FMIN, FMAX, SQRT, DIV, RCP, DOT, CROSS, MIXED, LEN, NORMALIZE, TRANSFORM, VDIV, VDIVS,
 RNG_SEED, RAND, SELFTEST) = range(24)

F32, U32, I32 = np.float32, np.uint32, np.int32
PTR = C.c_void_p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(PTR)


def _dev(hip_debug, op, n, a, b=None, c=None, out0=None, out1=None):
    fn = hip_debug.lib.jade_debug_fpmath
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int32, PTR, PTR, PTR, PTR, PTR]
    hip_debug.check(fn(0, op, n, _ptr(a), _ptr(b), _ptr(c), _ptr(out0), _ptr(out1)))


def _host(fpm, name, *args):
    fn = getattr(fpm, name)
    fn.restype = None
    fn.argtypes = [PTR if isinstance(a, np.ndarray) else C.c_int for a in args]
    fn(*[_ptr(a) if isinstance(a, np.ndarray) else a for a in args])


def _f(x):
    return np.ascontiguousarray(x, F32)


def assert_same_bits(got, want, what, *inputs):
    """Bit for bit equal, or both NaN.  inputs: the per-row input arrays, for the message."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, what
    g, w = got.reshape(-1).view(U32), want.reshape(-1).view(U32)
    bad = np.flatnonzero(~((g == w) | (np.isnan(got.reshape(-1)) & np.isnan(want.reshape(-1)))))
    if len(bad):
        width = max(len(g) // max(len(got), 1), 1)
        detail = [([np.asarray(x).reshape(len(x), -1)[i // width].tolist() for x in inputs], hex(g[i]), hex(w[i])) for i in bad[:5]]
        raise AssertionError(f"{what}: {len(bad)} of {len(g)} values differ; (inputs, got, want): {detail}")


def _nbrs(values):
    """Each value with its +-1 and +-2 ulp neighbours (and its negative's)."""
    v = _f(values)
    v = np.concatenate([v, -v])
    bits = v.view(U32).astype(np.int64)
    return np.concatenate([(bits + k).astype(U32) for k in (-2, -1, 0, 1, 2)]).view(F32)


ALL_EXPONENTS = (np.arange(1 << 20, dtype=U32) << 12).view(F32)  # every float whose low 12 mantissa bits are zero
_rng = np.random.default_rng(11)
_HALF_PI = np.concatenate([np.arange(0, 2048), np.arange(2048, 636620, 331)]).astype(np.float64) * (np.pi / 2)
# ^ multiples of pi/2 up to 1e6: all of the first 2048, then a SAMPLE, every 331st (all 636 620 with their neighbours would be 6.4 M
#   inputs; a test's input stays below 1.3 M)
UNARY = {
    # op: (host export, branch points, 200 k values of the integrator's own range)
    FLOOR: ("t_floor", [2147483648.0, 1.0, 0.5, 8388608.0, 16777216.0, 1e6], _rng.normal(size=200000) * 1e3),
    SINCOS: ("t_sincos", np.concatenate([_HALF_PI, [1e6, 0.78539816, 6.2831852]]),
             np.concatenate([_rng.random(150000) * 6.2831852, _rng.normal(size=50000) * 50])),
    LOG2: ("t_log2", [1.41421356, 2.0 ** -126, 1.0, 0.70710678, 2.0], np.exp(_rng.uniform(-60, 60, 200000))),
    EXP2: ("t_exp2", np.concatenate([[128.0, -149.0, -150.0, -126.0, 127.0], np.arange(-152, 130) + 0.5]), _rng.uniform(-155, 130, 200000)),
    ATAN: ("t_atan", [0.4142135623730950, 2.414213562373095, 1.0], _rng.normal(size=200000) * 10.0 ** _rng.uniform(-3, 3, 200000)),
    ASIN: ("t_asin", [0.5, 1.0], _rng.uniform(-1, 1, 200000)),
    SQRT: ("t_sqrt", [2.0 ** -126, 1.0, 2.0, 4.0], np.exp(_rng.uniform(-87, 87, 200000))),
    RCP: ("t_rcp", [2.0 ** -126, 1.0, 2.0 ** 126, 2.0 ** 127, 3.0], np.exp(_rng.uniform(-87, 87, 200000)) * _rng.choice([-1, 1], 200000)),
}


@pytest.mark.parametrize("op", sorted(UNARY), ids=lambda o: UNARY[o][0])
def test_unary_ops_equal_the_host_bits(hip_debug, fpm, op):
    name, points, own = UNARY[op]
    x = np.concatenate([ALL_EXPONENTS, _nbrs(points), _f(own)])
    assert len(x) <= 1300000
    n = len(x)
    got, got1 = np.empty(n, F32), np.empty(n, F32)
    want, want1 = np.empty(n, F32), np.empty(n, F32)
    if op == SINCOS:
        _dev(hip_debug, op, n, x, out0=got, out1=got1)
        _host(fpm, name, x, want, want1, n)
        assert_same_bits(got1, want1, "cos", x)
    else:
        _dev(hip_debug, op, n, x, out0=got)
        _host(fpm, name, x, want, n)
    assert_same_bits(got, want, name, x)
    with np.errstate(all="ignore"):  # IEEE, independent of the header and of the host's flags
        if op == SQRT:
            assert_same_bits(got, np.sqrt(x), "sqrt against IEEE", x)
        if op == RCP:
            assert_same_bits(got, F32(1.0) / x, "1 / a against IEEE", x)


def _specials():
    """About 200 values: zeros, subnormals, the edges of the normal range, neighbours of 1, infinities, NaN, the integrator's own
    exponents (1 / 2.2, float(JADE_E_D)), small integers and half-integers, powers of two across the range."""
    one = F32(1.0)
    pos = [0.0, 1e-45, 1.17549421e-38, 1.17549435e-38, np.nextafter(one, F32(0)), 1.0, np.nextafter(one, F32(2)), 3.40282347e38, np.inf,
           1.0 / 2.2, 2.71828182846, 2.2, 0.5, 1.5, 2.0, 2.5, 3.0, 4.0, 7.0, 10.0, 255.0, 3.14159265, 1.57079633, 0.9, 0.1, 1e-3, 1e-7,
           1e-20, 1e-30, 1e-37, 1e10, 1e20, 1e30, 1e38, 16777216.0, 2147483648.0, 4294967296.0, 0.41421356, 2.41421356, 0.70710678,
           1.41421356, 126.0, 127.0, 128.0, 149.0, 150.0]
    pos += [2.0 ** e for e in range(-148, 128, 6)]
    v = _f(pos)
    return np.concatenate([v, -v, [np.nan]]).astype(F32)


SPECIALS = _specials()
BINARY = {POW: "t_pow", ATAN2: "t_atan2", FMIN: "t_fmin_n", FMAX: "t_fmax_n", DIV: "t_div"}


def _binary(hip_debug, fpm, op, a, b):
    a, b = _f(a), _f(b)
    n = len(a)
    got, want = np.empty(n, F32), np.empty(n, F32)
    _dev(hip_debug, op, n, a, b, out0=got)
    _host(fpm, BINARY[op], a, b, want, n)
    assert_same_bits(got, want, BINARY[op], a, b)
    return got


@pytest.mark.parametrize("op", sorted(BINARY), ids=lambda o: BINARY[o])
def test_binary_ops_on_the_cross_product_of_special_values(hip_debug, fpm, op):
    assert 150 <= len(SPECIALS) <= 250
    a, b = [m.ravel() for m in np.meshgrid(SPECIALS, SPECIALS, indexing="ij")]
    got = _binary(hip_debug, fpm, op, a, b)
    if op == DIV:
        with np.errstate(all="ignore"):
            assert_same_bits(got, a / b, "a / b against IEEE", a, b)


def test_binary_ops_in_the_integrators_ranges(hip_debug, fpm):
    rng = np.random.default_rng(12)
    n = 200000
    _binary(hip_debug, fpm, POW, rng.random(n), np.full(n, 1.0 / 2.2))                 # the gamma curve
    _binary(hip_debug, fpm, POW, np.full(n, 2.71828182846), rng.uniform(-20, 0, n))    # the BSSRDF profile
    _binary(hip_debug, fpm, POW, rng.uniform(1e-6, 1, n), rng.uniform(0, 50, n))       # rate ^ distance
    _binary(hip_debug, fpm, ATAN2, rng.normal(size=n), rng.normal(size=n))
    tiny = 10.0 ** rng.uniform(-45, -30, n) * rng.choice([-1, 1], n)
    half = n // 2
    _binary(hip_debug, fpm, ATAN2, np.concatenate([tiny[:half], rng.normal(size=n - half)]),
            np.concatenate([rng.normal(size=half), tiny[half:]]))
    a = np.exp(rng.uniform(-87, 87, n)) * rng.choice([-1, 1], n)
    b = np.exp(rng.uniform(-87, 87, n)) * rng.choice([-1, 1], n)
    got = _binary(hip_debug, fpm, DIV, a, b)
    with np.errstate(all="ignore"):
        assert_same_bits(got, _f(a) / _f(b), "a / b against IEEE", _f(a), _f(b))


def test_fmin_fmax_signed_zero_and_nan_table_on_the_device(hip_debug):
    """The header's comment, on the device: a NaN operand is dropped, a tie returns the FIRST operand - so the sign of a zero result
    is the first operand's, where a hardware min / max instruction orders -0 below +0."""
    nan, pz, nz = F32(np.nan), F32(0.0), F32(-0.0)
    #          a    b     fmin  fmax
    table = [(pz, nz, pz, pz), (nz, pz, nz, nz), (pz, pz, pz, pz), (nz, nz, nz, nz), (nan, 2.0, 2.0, 2.0), (2.0, nan, 2.0, 2.0),
             (nan, nz, nz, nz), (nz, nan, nz, nz), (nan, nan, nan, nan), (1.0, 2.0, 1.0, 2.0), (2.0, 1.0, 1.0, 2.0),
             (-np.inf, np.inf, -np.inf, np.inf), (nan, np.inf, np.inf, np.inf), (-np.inf, nan, -np.inf, -np.inf), (1e-45, -1e-45, -1e-45, 1e-45)]
    a, b, lo, hi = [_f(col) for col in zip(*table)]
    for op, want in ((FMIN, lo), (FMAX, hi)):
        got = np.empty(len(a), F32)
        _dev(hip_debug, op, len(a), a, b, out0=got)
        assert_same_bits(got, want, "fmin" if op == FMIN else "fmax", a, b)


def test_vector_ops_equal_the_host_bits(hip_debug, fpm):
    """Rows of random vectors, and the same rows scaled so that products become subnormal (1e-20) or overflow (1e19)."""
    rng = np.random.default_rng(13)
    base = [rng.normal(size=(100000, 3)) for _ in range(3)]
    a, b, c = [_f(np.concatenate([v, v * 1e-20, v * 1e19])) for v in base]
    s = _f(np.concatenate([rng.normal(size=100000)] * 3) * np.repeat([1.0, 1e-20, 1e19], 100000))
    m = _f(rng.normal(size=16))
    n = len(a)
    cases = [(DOT, "t_dot_n", (a, b), 1), (CROSS, "t_cross_n", (a, b), 3), (MIXED, "t_mixed_n", (a, b, c), 1), (LEN, "t_len_n", (a,), 1),
             (NORMALIZE, "t_normalize_n", (a,), 3), (TRANSFORM, "t_transform_n", (a, s, m), 3), (VDIV, "t_vdiv_n", (a, b), 3),
             (VDIVS, "t_vdivs_n", (a, s), 3)]
    for op, name, ins, width in cases:
        got, want = np.empty((n, width), F32), np.empty((n, width), F32)
        _dev(hip_debug, op, n, *ins, out0=got)
        _host(fpm, name, *ins, want, n)
        assert_same_bits(got, want, name, *[x for x in ins if len(x) == n])
    with np.errstate(all="ignore"):  # jv_div / jv_divs are plain IEEE divisions
        got = np.empty((n, 3), F32)
        _dev(hip_debug, VDIV, n, a, b, out0=got)
        assert_same_bits(got, a / b, "jv_div against IEEE", a, b)
        _dev(hip_debug, VDIVS, n, a, s, out0=got)
        assert_same_bits(got, a / s[:, None], "jv_divs against IEEE", a, s)


# ---- the RNG: shaders/fshader_render.fsh:82-98 in Python integers, and its inverse (every step of the Wang hash is invertible)

M32 = 0xFFFFFFFF


def _wang(s):
    s = ((s ^ 61) ^ (s >> 16)) & M32
    s = (s * 9) & M32
    s = s ^ (s >> 4)
    s = (s * 0x27d4eb2d) & M32
    return s ^ (s >> 15)


def _unxorshift(v, k):
    s = v
    for _ in range(32 // k + 1):
        s = v ^ (s >> k)
    return s


def _unwang(h):
    s = _unxorshift(h, 15)
    s = (s * pow(0x27d4eb2d, -1, 1 << 32)) & M32
    s = _unxorshift(s, 4)
    s = (s * pow(9, -1, 1 << 32)) & M32
    hi = s >> 16
    return (hi << 16) | ((s & 0xFFFF) ^ 61 ^ hi)


def _rand(hip_debug, fpm, seeds, k):
    seeds = np.ascontiguousarray(seeds, U32)
    n = len(seeds)
    u, st = np.empty((n, k), F32), np.empty((n, k), U32)
    _dev(hip_debug, RAND, n, seeds, np.array([k], I32), out0=u, out1=st)
    hu, hst = np.empty((n, k), F32), np.empty((n, k), U32)
    _host(fpm, "t_rand_n", seeds, k, hu, hst, n)
    assert np.array_equal(st, hst) and np.array_equal(u.view(U32), hu.view(U32))
    return u, st


def test_rng_streams_and_the_uint_to_float_conversion(hip_debug, fpm):
    rng = np.random.default_rng(14)
    px, py, fr = [rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(U32) for _ in range(3)]
    px[:2048] %= 4096
    py[:2048] %= 4096
    fr[:2048] %= 100000
    seeds, want = np.empty(4096, U32), np.empty(4096, U32)
    _dev(hip_debug, RNG_SEED, 4096, px, py, fr, out0=seeds)
    _host(fpm, "t_seed_n", px, py, fr, want, 4096)
    py_seeds = ((px.astype(np.uint64) * 1973 + py.astype(np.uint64) * 9277 + fr.astype(np.uint64) * 26699) & M32 | 1).astype(U32)
    assert np.array_equal(seeds, want) and np.array_equal(seeds, py_seeds)
    u, st = _rand(hip_debug, fpm, seeds, 64)
    # the states by Python integers (a sample of the streams), every draw by numpy's round-to-nearest-even uint32 -> float32
    for i in range(0, 4096, 64):
        s = int(seeds[i])
        for j in range(64):
            s = _wang(s)
            assert st[i, j] == s
    assert np.array_equal(u, st.astype(F32) * F32(2.0 ** -32))
    assert u.min() >= 0 and u.max() <= 1


def test_rng_crafted_states_reach_the_ends_of_the_unit_interval(hip_debug, fpm):
    """States whose hash is 0, 0xFFFFFFFF and the three values around the rounding tie below 2^32 (0xFFFFFF80 is halfway between
    0xFFFFFF00 and 2^32 and goes to the even one, 2^32): u == 1.0f is reachable, and u == 0 too."""
    targets = [0, 0xFFFFFFFF, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFF81, 1, 0x80000000, 0x7FFFFFC0, 0x01000001]
    states = [_unwang(h) for h in targets]
    assert [_wang(s) for s in states] == targets
    u, st = _rand(hip_debug, fpm, np.array(states, U32), 2)
    assert st[:, 0].tolist() == targets and st[:, 1].tolist() == [_wang(h) for h in targets]
    below_one = F32(0xFFFFFF00) * F32(2.0 ** -32)
    assert below_one == F32(1.0) - F32(2.0 ** -24)
    want = [0.0, 1.0, below_one, 1.0, 1.0, 2.0 ** -32, 0.5, F32(0x7FFFFFC0) * F32(2.0 ** -32), F32(0x01000000) * F32(2.0 ** -32)]
    assert u[:, 0].tolist() == [float(w) for w in want]


def test_selftest_on_the_device(hip_debug, fpm):
    one = np.ones(256, F32)
    got = np.full(256, -1, I32)
    _dev(hip_debug, SELFTEST, 256, one, out0=got)
    assert (got == 0).all(), "the device code was built with FMA contraction, or without FMA"
    want = np.full(256, -1, I32)
    _host(fpm, "t_selftest_n", one, want, 256)
    assert (want == 0).all()


def test_float_to_int_conversions_inside_floor_and_sincos(hip_debug, fpm):
    """(int32_t)x truncates toward zero on both sides: floor on every half-integer and integer around zero and around +-2^23,
    where a float still has a fraction bit, and the quadrant of sincos on both sides of each multiple of pi/2."""
    x = np.concatenate([np.arange(-4096, 4096) * 0.25, 8388608.0 + np.arange(-64, 64) * 0.5, -8388608.0 + np.arange(-64, 64) * 0.5,
                        2147483648.0 - np.arange(0, 64) * 128.0, -2147483648.0 + np.arange(0, 64) * 128.0])
    x = _f(x)
    got, want = np.empty(len(x), F32), np.empty(len(x), F32)
    _dev(hip_debug, FLOOR, len(x), x, out0=got)
    assert_same_bits(got, np.floor(x), "floor against numpy", x)
    _host(fpm, "t_floor", x, want, len(x))
    assert_same_bits(got, want, "floor", x)
