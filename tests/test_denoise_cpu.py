"""The denoiser without a GPU: the numpy statement (tests/denoise_ref.py) on hand-derived cases, the entry points exported and
declared, and the oracle refusing them (Python and CLI)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import B, ORACLE_LIB, ROOT, config_scene
from jaderaytracerendering_amd import _abi

from denoise_ref import H5, denoise

NEW = ("jade_denoise_defaults", "jade_render_guides", "jade_render_denoise", "jade_denoise_image")
CLI = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "jade_render")


def _flat(h, w, value=0.5):
    """Equal guides everywhere: albedo, an upward normal, depth 1."""
    alb = np.full((h, w, 3), value)
    nrm = np.zeros((h, w, 3))
    nrm[..., 2] = 1.0
    return alb, nrm, np.ones((h, w))


def test_impulse_response_is_the_b3_kernel():
    h = w = 21
    rgb = np.zeros((h, w, 3))
    rgb[10, 10] = 1.0
    alb, nrm, dep = _flat(h, w)
    var = np.full((h, w), 1e12)  # w_l = exp(-|dl| / (4e6)): 1 to 3e-7
    out, _ = denoise(rgb, var, alb, nrm, dep, 1, 4.0, 128.0, 0.1, 0.1)
    want = np.zeros((h, w))
    want[8:13, 8:13] = np.outer(H5, H5)
    np.testing.assert_allclose(out[..., 0], want, atol=1e-6)
    # two passes: the B3 kernel convolved with itself dilated by 2 (every tap in the image: no renormalisation)
    out2, _ = denoise(rgb, var, alb, nrm, dep, 2, 4.0, 128.0, 0.1, 0.1)
    k1 = np.outer(H5, H5)
    k2 = np.zeros((9, 9))
    k2[::2, ::2] = k1
    full = np.zeros((13, 13))
    for i in range(5):
        for j in range(5):
            full[i:i + 9, j:j + 9] += k1[i, j] * k2
    want2 = np.zeros((h, w))
    want2[4:17, 4:17] = full
    np.testing.assert_allclose(out2[..., 0], want2, atol=1e-6)


def test_opposite_normals_keep_the_halves_apart():
    h, w = 12, 16
    rng = np.random.default_rng(3)
    rgb = rng.random((h, w, 3))
    alb, nrm, dep = _flat(h, w)
    nrm[:, w // 2:, 2] = -1.0
    var = rng.random((h, w))
    # one pass: the next pass's 3x3 variance blur (no edge stopping) carries the other half's filtered variance across the edge
    a, _ = denoise(rgb, var, alb, nrm, dep, 1, 4.0, 128.0, 0.1, 0.1)
    rgb2 = rgb.copy()
    rgb2[:, w // 2:] = rng.random((h, w - w // 2, 3)) * 10
    b, _ = denoise(rgb2, var, alb, nrm, dep, 1, 4.0, 128.0, 0.1, 0.1)
    assert np.array_equal(a[:, :w // 2], b[:, :w // 2])


def test_zero_iterations_and_constant_colour():
    h, w = 9, 7
    rng = np.random.default_rng(4)
    rgb = rng.random((h, w, 3))
    alb, nrm, dep = rng.random((h, w, 3)), rng.normal(size=(h, w, 3)), rng.random((h, w)) + 0.5
    var = rng.random((h, w))
    out, v = denoise(rgb, var, alb, nrm, dep, 0, 4.0, 128.0, 0.1, 0.1)
    assert np.array_equal(out, rgb) and np.array_equal(v, var)
    const = np.broadcast_to([0.2, 0.5, 0.9], (h, w, 3))
    out, _ = denoise(const, var, alb, nrm, dep, 4, 4.0, 128.0, 0.1, 0.1)
    np.testing.assert_allclose(out, const, rtol=1e-12)


def test_hip_library_exports_the_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", B.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    for n in NEW:
        assert n in names
    assert not {n for n in names if n.startswith("denoise_")}  # the launch helpers stay inside the library


def test_header_declares_them_with_the_formulas():
    text = open(os.path.join(ROOT, "include", "jade_bvh.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, text), n
    for line in ("v = sum (Y_l - m)^2 / (K (K - 1))", "w_l = exp(-|l_p - l_q| / (sigma_luminance sqrt(g_p) + 1e-10))",
                 "w_z = exp(-|z_p - z_q| / (sigma_depth max(z_p, z_q) + 1e-10))", "c'_p = sum w c_q / sum w"):
        assert line in text, line
    rt = open(os.path.join(ROOT, "include", "jade_rt.h")).read()
    assert "denoise" not in rt
    lib = ctypes.CDLL(B.HIP_LIB)
    _abi.bind(lib, {n: _abi.BVH_SYMBOLS[n] for n in NEW})
    assert ctypes.sizeof(_abi.DenoiseParams) == 24


def test_python_raises_unsupported_on_the_oracle(oracle):
    hs, cfg = config_scene("tiny")
    p = B.params_from_config(cfg, spp=4)
    p.width, p.height = 16, 16
    with oracle.scene(hs) as sc:
        sc.begin(p)
        sc.step(4)
        for call in (lambda: sc.denoise(), lambda: sc.guides()):
            with pytest.raises(B.JadeError) as e:
                call()
            assert e.value.code == _abi.JADE_ERR_UNSUPPORTED
    z = np.zeros((4, 4, 3), np.float32)
    with pytest.raises(B.JadeError) as e:
        oracle.denoise_image(z, z[..., 0], z, z, z[..., 0])
    assert e.value.code == _abi.JADE_ERR_UNSUPPORTED


@pytest.mark.parametrize("flags", [("--denoise",), ("--guides", "g")])
def test_cli_on_the_oracle_exits_2_naming_the_hip_backend(flags, tmp_path):
    r = subprocess.run([CLI, "--config", "tiny", "--width", "32", "--height", "32", "--spp", "4", "--backend", ORACLE_LIB,
                        "--out", str(tmp_path / "o.pfm"), *flags], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 2, r.stderr
    assert "needs the HIP backend" in r.stderr and "jade_render_denoise" in r.stderr
    assert "Start..." not in r.stdout
