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
