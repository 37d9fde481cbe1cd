"""Exposure without a GPU: the entry points declared and exported, the defaults, the policy (jade_meter_exposure - host code, no HIP
call) against the float64 statement of tests/exposure_spec.py, its refusals, and the CLI's."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import B, J, ORACLE_LIB, ROOT
from jaderaytracerendering_amd import _abi

import exposure_spec as X

NEW = ("jade_display_defaults", "jade_meter_exposure", "jade_render_meter", "jade_render_resolve_exposed", "jade_expose_image")
CLI = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "jade_render")


@pytest.fixture(scope="module")
def lib():
    return J.hip()  # (loading the library and calling its host code needs no device)


def auto(lib, key=0.18, p_lo=0.05, p_hi=0.95, min_exposure=2.0 ** -16, max_exposure=2.0 ** 16):
    p = lib.display_defaults()
    p.exposure_mode = _abi.EXPOSURE_AUTO
    p.key, p.p_lo, p.p_hi, p.min_exposure, p.max_exposure = key, p_lo, p_hi, min_exposure, max_exposure
    return p


def meter_of(bins):
    full = np.zeros(X.BINS, np.uint64)
    for b, n in bins.items():
        full[b] = n
    return B.Meter(full)


def close(got, want):
    return abs(float(got) - float(want)) <= X.POLICY_RTOL * abs(float(want))


def test_the_header_declares_and_the_library_exports_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jade_bvh.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", B.HIP_LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert n in names, n
        assert n in _abi.BVH_SYMBOLS
    assert "#define JADE_METER_BINS 512" in text and _abi.METER_BINS == 512
    assert not {n for n in names if n.startswith(("ex_", "meter_"))}  # the helpers stay inside the library


def test_display_defaults(lib):
    p = lib.display_defaults()
    assert (p.tonemap, p.exposure_mode, p.exposure) == (_abi.TONEMAP_ACES, _abi.EXPOSURE_MANUAL, 1.0)
    assert (p.key, p.p_lo, p.p_hi) == (float(np.float32(0.18)), float(np.float32(0.05)), float(np.float32(0.95)))
    assert (p.min_exposure, p.max_exposure) == (2.0 ** -16, 2.0 ** 16)


def test_manual_returns_the_multiplier(lib):
    p = lib.display_defaults()
    p.exposure = 0.37
    assert lib.meter_exposure(None, p) == float(np.float32(0.37))
    assert lib.meter_exposure(meter_of({3: 5}), p) == float(np.float32(0.37))


def test_single_bin_at_one(lib):
    """Bin 256 is [1, 1.125): its centre is 1.0625 whatever the window, so e = key / 1.0625."""
    for window in ((0.05, 0.95), (0.0, 1.0), (0.4, 0.6)):
        e = lib.meter_exposure(meter_of({256: 1000}), auto(lib, 0.18, *window))
        assert close(e, np.float64(np.float32(0.18)) / 1.0625), (window, e)
        assert close(e, X.exposure(meter_of({256: 1000}).bins, 0.18, *window))


def test_a_window_that_cuts_a_bin_in_half(lib):
    """100 pixels in bin 256 and 100 in bin 264 (one stop up), window [0, 0.75]: the weights are 100 and 50."""
    m = meter_of({256: 100, 264: 100})
    l0 = math.log2(1.0625)
    want = np.float64(np.float32(0.5)) * 2.0 ** -((100 * l0 + 50 * (1 + l0)) / 150)
    e = lib.meter_exposure(m, auto(lib, 0.5, 0.0, 0.75))
    assert close(e, want) and close(e, X.exposure(m.bins, 0.5, 0.0, 0.75))
    # ... and from the other side, [0.25, 1]: 50 and 100
    want = np.float64(np.float32(0.5)) * 2.0 ** -((50 * l0 + 100 * (1 + l0)) / 150)
    assert close(lib.meter_exposure(m, auto(lib, 0.5, 0.25, 1.0)), want)


def test_the_full_window_is_the_log_average(lib):
    bins = {0: 7, 100: 1, 255: 300, 256: 12, 300: 1000, 511: 3}
    c = X.bin_centre_log2()
    log_avg = sum(n * c[b] for b, n in bins.items()) / sum(bins.values())
    e = lib.meter_exposure(meter_of(bins), auto(lib, 0.18, 0.0, 1.0))
    assert close(e, np.float64(np.float32(0.18)) * 2.0 ** -log_avg)
    assert close(e, X.exposure(meter_of(bins).bins, 0.18, 0.0, 1.0))


def test_the_empty_meter_gives_one_then_the_clamp(lib):
    assert lib.meter_exposure(B.Meter(), auto(lib)) == 1.0
    assert lib.meter_exposure(B.Meter(n_zero=50, n_negative=2, n_nonfinite=1), auto(lib)) == 1.0  # (only positive pixels are metered)
    assert lib.meter_exposure(B.Meter(), auto(lib, min_exposure=2.0, max_exposure=4.0)) == 2.0
    assert lib.meter_exposure(B.Meter(), auto(lib, min_exposure=0.125, max_exposure=0.5)) == 0.5


def test_both_clamps(lib):
    dark, bright = meter_of({8: 10}), meter_of({500: 10})  # around 2^-31 and 2^30
    assert lib.meter_exposure(dark, auto(lib)) == 2.0 ** 16
    assert lib.meter_exposure(bright, auto(lib)) == 2.0 ** -16
    assert lib.meter_exposure(dark, auto(lib, min_exposure=0.5, max_exposure=8.0)) == 8.0
    assert lib.meter_exposure(bright, auto(lib, min_exposure=0.5, max_exposure=8.0)) == 0.5
    assert lib.meter_exposure(bright, auto(lib, min_exposure=3.0, max_exposure=3.0)) == 3.0


def test_random_meters_against_the_float64_statement(lib):
    rng = np.random.default_rng(7)
    worst = 0.0
    for i in range(2000):
        bins = np.zeros(X.BINS, np.uint64)
        occupied = rng.choice(X.BINS, int(rng.integers(1, 60 if i % 3 else X.BINS)), replace=False)
        bins[occupied] = (10.0 ** rng.uniform(0, 9 if i % 5 else 14, len(occupied))).astype(np.uint64)
        lo = float(rng.uniform(0, 0.9)) if i % 4 else 0.0
        hi = float(rng.uniform(lo + 0.01, 1.0)) if i % 7 else 1.0
        key = float(10.0 ** rng.uniform(-2, 1))
        clamp = (2.0 ** -16, 2.0 ** 16) if i % 2 else (float(2.0 ** rng.uniform(-40, 0)), float(2.0 ** rng.uniform(0, 40)))
        want = X.exposure(bins, key, lo, hi, *clamp)
        got = lib.meter_exposure(B.Meter(bins), auto(lib, key, lo, hi, *clamp))
        assert close(got, want), (i, got, want, lo, hi, key, clamp)
        worst = max(worst, abs(got - float(want)) / float(want))
    print(f"largest relative difference over 2000 random meters: {worst:.3g} (bound {X.POLICY_RTOL})")


BAD = [
    ("mode", dict(exposure_mode=2)), ("mode", dict(exposure_mode=-1)),
    ("exposure", dict(exposure_mode=0, exposure=0.0)), ("exposure", dict(exposure_mode=0, exposure=-1.0)),
    ("exposure", dict(exposure_mode=0, exposure=math.nan)), ("exposure", dict(exposure_mode=0, exposure=math.inf)),
    ("key", dict(key=0.0)), ("key", dict(key=-0.18)), ("key", dict(key=math.nan)), ("key", dict(key=math.inf)),
    ("window", dict(p_lo=-0.1)), ("window", dict(p_lo=0.5, p_hi=0.5)), ("window", dict(p_lo=0.6, p_hi=0.4)), ("window", dict(p_hi=1.5)),
    ("window", dict(p_lo=math.nan)), ("window", dict(p_hi=math.nan)),
    ("clamp", dict(min_exposure=0.0)), ("clamp", dict(min_exposure=2.0, max_exposure=1.0)), ("clamp", dict(max_exposure=math.inf)),
    ("clamp", dict(min_exposure=math.nan)), ("clamp", dict(min_exposure=-1.0)),
]


@pytest.mark.parametrize("word,fields", BAD, ids=[f"{w}-{i}" for i, (w, _) in enumerate(BAD)])
def test_each_invalid_parameter_gives_nan_and_a_message(lib, word, fields):
    p = auto(lib)
    for k, v in fields.items():
        setattr(p, k, v)
    fn = lib.hip_only("jade_meter_exposure")
    m = meter_of({256: 10}).to_struct()
    e = fn(m, p)
    assert math.isnan(e)
    assert word in lib.lib.jade_last_error().decode()
    with pytest.raises(B.JadeError) as ei:
        lib.meter_exposure(meter_of({256: 10}), p)
    assert ei.value.code == _abi.JADE_ERR_INVALID


def test_null_pointers_give_nan(lib):
    fn = lib.hip_only("jade_meter_exposure")
    assert math.isnan(fn(meter_of({256: 10}).to_struct(), None)) and "null" in lib.lib.jade_last_error().decode()
    assert math.isnan(fn(None, auto(lib))) and "null" in lib.lib.jade_last_error().decode()


def test_meter_class_adds_and_knows_its_edges():
    a = B.Meter(meter_of({3: 1, 256: 5}).bins, 1, 2, 3, 0.25, 1.0)
    b = B.Meter(meter_of({256: 2, 400: 1}).bins, 10, 0, 0, 1.0, 7.0e5)
    s = a + b
    assert s.bins[256] == 7 and s.n_positive == 9 and s.total == 9 + 16
    assert (s.n_zero, s.n_negative, s.n_nonfinite, float(s.lum_min), float(s.lum_max)) == (11, 2, 3, 0.25, 7.0e5)
    assert (a + B.Meter(n_zero=4)).lum_min == np.float32(0.25)  # a rank without positive pixels does not bring its 0 in
    assert a + B.Meter() == a and a != b
    edges = B.Meter.bin_edges()
    assert edges[0] == 2.0 ** -32 and edges[256] == 1.0 and edges[257] == 1.125 and edges[512] == 2.0 ** 32
    # the spec puts every edge, taken as a grey pixel, into the bin that starts there
    grey = np.repeat(edges[:-1].astype(np.float32).reshape(-1, 1), 3, 1)
    assert np.array_equal(X.classify(grey)[2], np.arange(X.BINS))


def test_cli_on_the_oracle_exits_2_naming_the_hip_backend(tmp_path):
    for flags in (("--exposure", "auto"), ("--exposure", "-1.5"), ("--histogram", "h.txt")):
        r = subprocess.run([CLI, "--config", "tiny", "--width", "32", "--height", "32", "--spp", "4", "--backend", ORACLE_LIB,
                            "--out", str(tmp_path / "o.bmp"), *flags], capture_output=True, text=True, timeout=300, cwd=tmp_path)
        assert r.returncode == 2, r.stderr
        assert "needs the HIP backend" in r.stderr and "jade_render_resolve_exposed" in r.stderr
        assert "Start..." not in r.stdout


@pytest.mark.parametrize("flags", [("--exposure", "x"), ("--exposure", "1e999"), ("--exposure", "100"), ("--exposure",),
                                   ("--exposure", "auto", "--key", "0"), ("--exposure", "auto", "--key", "k"),
                                   ("--exposure", "auto", "--exposure-window", "0.5"), ("--exposure", "auto", "--exposure-window", "0.9,0.1"),
                                   ("--exposure", "auto", "--exposure-window", "0,1.5"), ("--exposure", "auto", "--exposure-window", "a,b"),
                                   ("--exposure", "1", "--key", "0.2"), ("--key", "0.2")])
def test_cli_rejects_malformed_values_before_building_a_scene(flags, tmp_path):
    r = subprocess.run([CLI, "--config", "tiny", "--backend", ORACLE_LIB, *flags], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr, (r.returncode, r.stderr)
    assert "Model load done" not in r.stdout
