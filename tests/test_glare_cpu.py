"""Glare without a GPU: the entry points declared and exported, the defaults, the properties of the float64 statement
(tests/glare_ref.py) that the device tests then lean on, the refusals of jade_glare_image (made before any HIP call), and the CLI's."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import B, J, ORACLE_LIB, ROOT, rel_l2
from jaderaytracerendering_amd import _abi

import glare_cases as K
import glare_ref as G

NEW = ("jade_glare_defaults", "jade_glare_image", "jade_render_glare")
CLI = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "jade_render")


@pytest.fixture(scope="module")
def lib():
    return J.hip()  # (loading the library and calling its host code needs no device)


def test_the_header_declares_and_the_library_exports_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jade_bvh.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", B.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert n in names, n
        assert n in _abi.BVH_SYMBOLS
    # the helpers stay inside the library; they are C++, so an exported one would show mangled: ask nm for the plain names
    plain = subprocess.run(["nm", "-D", "-C", "--defined-only", B.HIP_LIB], capture_output=True, text=True, check=True).stdout
    leaked = [line for line in plain.splitlines() if re.search(r"\s(gl_|ex_|meter_)\w*\(", line)]
    assert not leaked, leaked
    assert re.search(r"\sk_gl_reduce\(", plain)  # (the pattern does see this library's C++ names: a kernel's host handle)
    assert "#define JADE_ABI_VERSION 7" in open(os.path.join(ROOT, "include", "jade_rt.h")).read()  # no existing struct or signature changed


def test_glare_defaults(lib):
    p = lib.glare_defaults()
    assert (p.levels, p.strength, p.falloff) == (6, float(np.float32(0.1)), 0.5)
    assert C.sizeof(_abi.GlareParams) == 12


def test_the_oracle_has_none_of_it(oracle):
    for n in NEW:
        assert not hasattr(oracle.lib, n), n
    with pytest.raises(B.JadeError) as e:
        oracle.glare_defaults()
    assert e.value.code == _abi.JADE_ERR_UNSUPPORTED
    with pytest.raises(B.JadeError) as e:
        oracle.glare_image(np.ones((2, 2, 3), np.float32))
    assert e.value.code == _abi.JADE_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------- the statement's own properties --

SHAPES = ((1, 1), (24, 17), (33, 20), (7, 40), (257, 3))  # (H, W)


def _random(rng, h, w):
    """colours over six decades"""
    return (rng.random((h, w, 3)) * 10.0 ** rng.uniform(-3, 3, (h, w, 1))).astype(np.float32)


def test_level_sizes_and_weights():
    assert G.level_sizes(27, 45, 7) == [(27, 45), (14, 23), (7, 12), (4, 6), (2, 3), (1, 2), (1, 1), (1, 1)]
    w = G.weights(4, 0.5)
    assert np.allclose(w, np.array([8, 4, 2, 1]) / 15.0, rtol=1e-15) and abs(w.sum() - 1) < 1e-15
    assert np.array_equal(G.weights(1, 0.3), [1.0])
    assert np.allclose(G.weights(3, 2.0), np.array([1, 2, 4]) / 7.0, rtol=1e-15)


def test_a_constant_frame_stays_constant():
    for h, w in SHAPES + ((27, 45),):
        for levels in (1, 3, 12):
            k = np.full((h, w, 3), 0.7, np.float32)
            for dt, tol in ((np.float64, 1e-12), (np.float32, 1e-6)):
                out = G.glare(k, levels, 0.3, 0.5, dt)
                assert np.abs(out / np.float64(np.float32(0.7)) - 1).max() <= tol, (h, w, levels, dt)


def test_an_impulse_keeps_its_sums_and_stays_clear_of_the_border():
    """What tests/test_gpu_glare.py's impulse test takes for granted: 3 levels reach 2 + 2*2 + 4*2 + ... pixels, well inside 96."""
    x = np.zeros((96, 96, 3), np.float32)
    x[48, 48] = (3.0, 1.0, 0.5)
    out = G.glare(x, 3, 0.4, 0.5)
    # (float32(0.4) + (1 - float32(0.4)) rounded to float32 is not exactly 1: two roundings of 6e-8 each)
    assert np.allclose(out.sum((0, 1)), x.sum((0, 1), dtype=np.float64), rtol=2e-7)
    assert np.allclose(G.glare(x, 3, 0.5, 0.5).sum((0, 1)), x.sum((0, 1), dtype=np.float64), rtol=1e-14)
    border = np.concatenate([out[0], out[-1], out[:, 0], out[:, -1]])
    assert not border.any()
    assert out[48, 48, 0] > 0.6 * 3.0 and (out >= 0).all()
    assert np.count_nonzero(out[..., 0]) > 25 * 25  # a halo, not a dot


def test_strength_zero_is_the_identity():
    x = np.float32([[[-0.0, 1e-45, np.nan], [np.inf, -np.inf, 3.4028235e38]]])
    for dt in (np.float64, np.float32):
        out = G.glare(x, 6, 0.0, 0.5, dt)
        assert out.dtype == np.float32 and out.tobytes() == x.tobytes()


def test_non_finite_pixels_pass_through_and_their_neighbours_stay_finite():
    rng = np.random.default_rng(3)
    x = _random(rng, 33, 20)
    x[4, 5, 1], x[0, 0, 0], x[32, 19, 2] = np.nan, np.inf, -np.inf
    bad = np.zeros((33, 20), bool)
    bad[4, 5] = bad[0, 0] = bad[32, 19] = True
    clean = np.where(bad[..., None], 0, x)
    for dt in (np.float64, np.float32):
        out = G.glare(x, 6, 0.3, 0.5, dt)
        assert np.array_equal(out[bad].astype(np.float32), x[bad], equal_nan=True)
        assert np.isfinite(out[~bad]).all()
        assert np.array_equal(out[~bad], G.glare(clean, 6, 0.3, 0.5, dt)[~bad])  # a bad pixel scatters as a black one


def test_the_operator_is_linear_in_the_frame():
    rng = np.random.default_rng(4)
    a, b = rng.random((20, 33, 3)), rng.random((20, 33, 3))
    ga, gb = G.glare(a, 4, 0.3, 0.5), G.glare(b, 4, 0.3, 0.5)
    assert rel_l2(G.glare(2.0 * a - 0.5 * b, 4, 0.3, 0.5), 2.0 * ga - 0.5 * gb) <= 1e-14
    # ... and in the strength: out = (1 - s) c + s B
    full = G.glare(a, 4, 1.0, 0.5)
    assert rel_l2(G.glare(a, 4, 0.25, 0.5), 0.75 * a + 0.25 * full) <= 1e-14


def test_float32_evaluates_the_statement_within_a_hundredth_of_the_tolerance():
    """The bound of the device tests, G.TOL = 1e-5, is about 200 times what the number format itself costs."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for h, w in SHAPES:
        for levels in (1, 3, 12):
            x = _random(rng, h, w)
            worst = max(worst, rel_l2(G.glare(x, levels, 0.3, 0.5, np.float32), G.glare(x, levels, 0.3, 0.5)))
    print(f"float32 against float64, worst relative L2: {worst:.3g}")
    assert worst <= G.TOL / 100


# --------------------------------------------------------------------------------- the float32 statement, held bit for bit --

def _longhand_weights(levels, f):
    """gl_run's lines, one for one: the powers relative to the largest when f > 1, the sum in increasing k, then the float"""
    k0 = levels if f > 1.0 else 1
    wd, wsum = {}, 0.0
    for k in range(1, levels + 1):
        wd[k] = math.pow(f, k - k0)
        wsum += wd[k]
    return np.array([np.float32(wd[k] / wsum) for k in range(1, levels + 1)], np.float32)


def _fits(f, levels):
    """f^(levels-1), and the sum of the powers up to it, in a double"""
    try:
        return math.pow(f, levels - 1) < 1.7e308 / levels
    except OverflowError:
        return False


def _old_weights(levels, falloff):
    """what this file's statement said before: f^(k-1) / sum, numpy's sum"""
    with np.errstate(all="ignore"):
        w = np.float64(falloff) ** np.arange(levels, dtype=np.float64)
        return w / w.sum()


def test_weights_are_finite_sum_to_one_and_are_the_librarys_formula():
    rng = np.random.default_rng(7)
    falloffs = [float(np.float32(f)) for f in K.FALLOFFS + (1.0000001, 0.99999994, 3.0, 0.3, 1e-20, 1e20)]
    falloffs += [float(f) for f in (10.0 ** rng.uniform(-45, 38.5, 400)).astype(np.float32) if f > 0]
    overflowed = 0
    for levels in range(1, 13):
        for f in falloffs:
            w = G.weights(levels, f)
            assert w.dtype == np.float64 and w.shape == (levels,)
            assert np.isfinite(w).all() and (w >= 0).all(), (levels, f, w)
            assert abs(math.fsum(w) - 1.0) <= 1e-15, (levels, f, math.fsum(w))
            assert np.array_equal(w.astype(np.float32).view(np.uint32), _longhand_weights(levels, f).view(np.uint32)), (levels, f)
            if _fits(f, levels):  # the mathematical meaning kept: where f^(k-1) does not overflow, the old weights
                assert np.abs(w - _old_weights(levels, f)).max() <= 1e-15, (levels, f)
            else:
                overflowed += 1
    assert overflowed > 0 and not np.isfinite(_old_weights(12, 1e30)).all()  # (what the old form did there)
    for f in (K.TINY, 1e-30, 1e30, K.F32_MAX):
        w = G.weights(12, float(np.float32(f)))
        assert np.isfinite(w).all() and abs(math.fsum(w) - 1.0) <= 1e-15, (f, w)
        assert w[0 if f < 1 else 11] == 1.0


def test_every_case_is_finite_in_the_statement_but_for_the_bad_pixels_it_passes_through():
    """A condition of the cases, not a tolerance: with a NaN in the statement, bit equality would compare NaN payloads that the
    header does not fix.  (+inf on the `top` frames is a result.)"""
    cases = K.CASES + [K.TALL_CASE] + [K.operator_case(*f, lv) for f in K.OPERATOR_FRAMES for lv in (1, 2)]
    seen = {k: set() for k in ("kind", "levels", "falloff", "strength", "shape")}
    infs = 0
    for c in cases:
        x, out = K.frame(c.kind, c.w, c.h), K.want(c)
        bad = K.bad_mask(x)
        assert bad.any() == (c.kind == "bad"), c.id
        assert not np.isnan(out[~bad]).any(), c.id
        assert np.array_equal(K.bits(out)[bad], K.bits(x)[bad]), c.id
        if c.kind != "top":
            assert np.isfinite(out[~bad]).all(), c.id
        infs += int(np.isposinf(out).sum())
        for k, v in (("kind", c.kind), ("levels", c.levels), ("falloff", c.falloff), ("strength", c.strength), ("shape", (c.w, c.h))):
            seen[k].add(v)
    print(f"{len(cases)} cases, {infs} +inf words on the `top` frames")
    assert seen["kind"] == set(K.KINDS) and seen["levels"] == set(K.LEVELS)
    assert seen["shape"] == set(K.SHAPES.values()) | {K.TALL}
    # the coverage that was asked for
    have = {(c.kind, c.w, c.h, c.falloff) for c in K.CASES}
    for wh in K.SHAPES.values():
        for kind in ("decades", "halo"):
            for f in (0.5, 2.0):
                assert (kind, *wh, f) in have, (kind, wh, f)
    for wh in K.SWEEP:
        assert {c.falloff for c in K.CASES if (c.w, c.h) == wh} == {float(np.float32(f)) for f in K.FALLOFFS}
        assert {c.strength for c in K.CASES if (c.w, c.h) == wh} == set(K.STRENGTHS)
    for wh in K.ALL_KINDS:
        assert {c.kind for c in K.CASES if (c.w, c.h) == wh} == set(K.KINDS)
    # the frames are what they are named for
    x = K.frame("signed", 65, 17)
    assert np.signbit(x[:12, :12]).all() and not x[:12, :12].any() and (x < 0).any() and (x > 0).any()
    d = np.abs(K.frame("denormal", 65, 17))
    assert d.min() >= K.TINY and d.max() <= 1.2e-38 and (d < 1.1754944e-38).mean() > 0.9
    t = K.frame("top", 131, 35)
    assert t.min() >= 0 and t.max() == np.float32(K.F32_MAX) and np.isfinite(t).all()
    b = K.bits(K.frame("bad", 131, 35))
    assert {int(b[y, xx, ch]) for y, xx, ch, _ in K.bad_pixels(35, 131)} >= {0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000}
    assert infs > 0


def test_the_sums_begin_with_their_first_product():
    """-0.0 everywhere: the device's first term is the product itself, so every sum of the pyramid is -0.0 (started at +0 it is +0.0)"""
    x = np.full((9, 11, 3), -0.0, np.float32)
    for levels in (1, 3):
        out = G.glare(x, levels, 1.0, 0.5, np.float32)
        assert np.signbit(out).all() and not out.any()


class _ClampEarly(G.Statement):
    """REDUCE clamps its upper source index one pixel early (still inside the level)"""
    def reduce_source(self, x, i, n):
        return np.clip(2 * x + i, 0, max(n - 2, 0))


class _ExpandLastOdd(G.Statement):
    """EXPAND takes a(j) for a(j+1) on the last odd index"""
    def expand_sources(self, x, m):
        lo, mid, hi = super().expand_sources(x, m)
        odd = x[x % 2 == 1]
        if len(odd):
            hi = np.where(x == odd[-1], mid, hi)
        return lo, mid, hi


class _OutsideIn(G.Statement):
    """a five-term sum added outside-in, (a + e) + (b + d) + c"""
    def add(self, terms, dt):
        if len(terms) != 5:
            return super().add(terms, dt)
        a, b, c, d, e = terms
        return (((a + e).astype(dt) + (b + d).astype(dt)).astype(dt) + c).astype(dt)


class _FromZero(G.Statement):
    """every sum started at +0"""
    def add(self, terms, dt):
        return super().add([np.zeros_like(terms[0])] + list(terms), dt)


class _OldWeights(G.Statement):
    """f^(k-1) / sum, as this file's statement said before"""
    def weights(self, levels, falloff):
        return _old_weights(levels, falloff)


class _OneMinusInDouble(G.Statement):
    """1 - s taken in double from the caller's s and then rounded (the float subtraction of the rounded s is what the header says)"""
    def one_minus(self, strength):
        return np.float32(strength), np.float32(1.0 - float(strength))


# (the break, whether its relative L2 against float64 on `halo` 67 x 35 at 3 levels is under the old bound G.TOL = 1e-5)
BREAKS = [(_ClampEarly, True), (_ExpandLastOdd, False), (_OutsideIn, True), (_FromZero, True), (_OldWeights, True), (_OneMinusInDouble, True)]


@pytest.mark.parametrize("cls,under", BREAKS, ids=[c.__name__.lstrip("_") for c, _ in BREAKS])
def test_a_one_line_break_of_the_statement_differs_in_bits_and_what_the_old_bound_made_of_it(cls, under):
    """The gap this file's bit-for-bit tests close, written down: each break keeps every index inside its level, each changes the
    bits of at least one case of tests/glare_cases.py, and the whole-image relative L2 of 1e-5 that the device was held to before
    accepts it on the frame glare is for (a bright centre on a dim ground owns the norm).  Statement only: no kernel is broken."""
    broken = cls()
    hit = None
    with np.errstate(all="ignore"):
        for c in K.CASES:
            out = broken.glare(K.frame(c.kind, c.w, c.h), c.levels, c.strength, c.falloff, np.float32)
            if not np.array_equal(K.bits(out), K.bits(K.want(c))):
                hit = (c.id, K.differences(out, K.want(c), 2))
                break
    assert hit is not None, f"{cls.__name__} changes no bit of any case"
    x = K.frame("halo", 67, 35)
    s = 0.6 if cls is _OneMinusInDouble else 0.3  # (at 0.3 this break is no break: both give 0.7f)
    want = G.glare(x, 3, s, 0.5)
    err = rel_l2(broken.glare(x, 3, s, 0.5, np.float32), want)
    base = rel_l2(G.glare(x, 3, s, 0.5, np.float32), want)
    print(f"{cls.__name__}: first differs on {hit[0]} ({hit[1][0]} pixels); halo 67x35, 3 levels: relative L2 {err:.3g} "
          f"(the statement in float32: {base:.3g}; the old bound {G.TOL})")
    assert (err <= G.TOL) == under
    assert base <= G.TOL / 100


def test_one_minus_s_in_double_is_no_break_when_s_is_already_a_float():
    """Why the table above takes 1 - s from the caller's double: for a float s in [0, 1] the double 1 - s is exact (or rounds to 1
    where the float does), so rounding it gives the float subtraction - at every strength of the cases and at random ones."""
    rng = np.random.default_rng(11)
    some = np.concatenate([np.float32(K.STRENGTHS), rng.random(100000).astype(np.float32), (10.0 ** rng.uniform(-45, 0, 1000)).astype(np.float32)])
    assert np.array_equal((1.0 - some.astype(np.float64)).astype(np.float32), np.float32(1.0) - some)


# ------------------------------------------------------------------------------------------------------------- refusals --

BAD = [("levels", dict(levels=0)), ("levels", dict(levels=13)), ("levels", dict(levels=-1)),
       ("strength", dict(strength=-0.1)), ("strength", dict(strength=1.5)), ("strength", dict(strength=math.nan)),
       ("strength", dict(strength=math.inf)),
       ("falloff", dict(falloff=0.0)), ("falloff", dict(falloff=-1.0)), ("falloff", dict(falloff=math.inf)), ("falloff", dict(falloff=math.nan))]


@pytest.mark.parametrize("word,fields", BAD, ids=[f"{w}-{i}" for i, (w, _) in enumerate(BAD)])
def test_each_invalid_parameter_is_refused_before_any_hip_call(lib, word, fields):
    """The first HIP call of jade_glare_image is the device count (jade_denoise_image's order): without a device it answers
    JADE_ERR_DEVICE, with one it refuses device 10^6 with a text about the device.  JADE_ERR_INVALID with the parameter's name in
    the text says the check came before either."""
    fn = lib.hip_only("jade_glare_image")
    p = lib.glare_defaults()
    for k, v in fields.items():
        setattr(p, k, v)
    img = np.ones((4, 5, 3), np.float32)
    out = np.zeros_like(img)
    assert fn(10 ** 6, 5, 4, img.ctypes.data, C.byref(p), out.ctypes.data) == _abi.JADE_ERR_INVALID  # (not the device's complaint)
    assert word in lib.lib.jade_last_error().decode()
    assert not out.any()
    with pytest.raises(B.JadeError) as e:
        lib.glare_image(img, p)
    assert e.value.code == _abi.JADE_ERR_INVALID


def test_null_pointers_and_bad_sizes_are_refused(lib):
    fn = lib.hip_only("jade_glare_image")
    ok = lib.glare_defaults()
    img = np.ones((4, 5, 3), np.float32)
    out = np.zeros_like(img)
    for args, word in (((0, 5, 4, None, C.byref(ok), out.ctypes.data), "null"), ((0, 5, 4, img.ctypes.data, C.byref(ok), None), "null"),
                       ((0, 5, 4, img.ctypes.data, None, out.ctypes.data), "null"), ((0, 0, 4, img.ctypes.data, C.byref(ok), out.ctypes.data), "size"),
                       ((0, 5, -1, img.ctypes.data, C.byref(ok), out.ctypes.data), "size"),
                       ((0, 1 << 20, 1 << 20, img.ctypes.data, C.byref(ok), out.ctypes.data), "size"),
                       ((0, 1, 16 * 65535 + 1, img.ctypes.data, C.byref(ok), out.ctypes.data), "size")):  # taller than the grids hold
        assert fn(*args) == _abi.JADE_ERR_INVALID, args
        assert word in lib.lib.jade_last_error().decode()
    assert not out.any()
    render = lib.hip_only("jade_render_glare")
    assert render(None, C.byref(ok), None, out.ctypes.data, None, None) == _abi.JADE_ERR_INVALID  # no scene, no render begun


# ------------------------------------------------------------------------------------------------------------------ CLI --

def test_cli_on_the_oracle_exits_2_naming_the_hip_backend(tmp_path):
    for flags in (("--glare", "0.2"), ("--glare", "0.2", "--glare-levels", "3", "--glare-falloff", "0.7"), ("--glare", "0")):
        r = subprocess.run([CLI, "--config", "tiny", "--width", "32", "--height", "32", "--spp", "4", "--backend", ORACLE_LIB,
                            "--out", str(tmp_path / "o.bmp"), *flags], capture_output=True, text=True, timeout=300, cwd=tmp_path)
        assert r.returncode == 2, r.stderr
        assert "needs the HIP backend" in r.stderr and "jade_render_glare" in r.stderr
        assert "Start..." not in r.stdout
    # the same status and style as --denoise
    d = subprocess.run([CLI, "--config", "tiny", "--width", "32", "--height", "32", "--spp", "4", "--backend", ORACLE_LIB,
                        "--out", str(tmp_path / "o.bmp"), "--denoise"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert d.returncode == 2 and "--denoise needs the HIP backend" in d.stderr and "--glare needs the HIP backend" in r.stderr


@pytest.mark.parametrize("flags", [("--glare", "x"), ("--glare", "-0.1"), ("--glare", "1.5"), ("--glare", "nan"), ("--glare",),
                                   ("--glare", "0.2", "--glare-levels", "0"), ("--glare", "0.2", "--glare-levels", "13"),
                                   ("--glare", "0.2", "--glare-levels", "2.5"), ("--glare", "0.2", "--glare-falloff", "0"),
                                   ("--glare", "0.2", "--glare-falloff", "-1"), ("--glare", "0.2", "--glare-falloff", "1e999"),
                                   ("--glare-levels", "3"), ("--glare-falloff", "0.5")])
def test_cli_rejects_malformed_values_before_building_a_scene(flags, tmp_path):
    r = subprocess.run([CLI, "--config", "tiny", "--backend", ORACLE_LIB, *flags], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr, (r.returncode, r.stderr)
    assert "Model load done" not in r.stdout


def test_cli_without_glare_is_unchanged_on_the_oracle(tmp_path):
    """No --glare: no glare symbol is looked up, and the oracle backend renders as before."""
    r = subprocess.run([CLI, "--config", "tiny", "--width", "32", "--height", "32", "--spp", "2", "--backend", ORACLE_LIB,
                        "--out", str(tmp_path / "o.bmp")], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "glare:" not in r.stdout and (tmp_path / "o.bmp").stat().st_size > 32 * 32 * 3
