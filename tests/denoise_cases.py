"""Small frames on which the denoiser's filter mixes (tests/test_denoise_cpu.py, tests/test_gpu_denoise_exact.py).

The "random" frames of tests/test_gpu_denoise.py have independent normals, so w_n is ~0 for every tap but the centre and the filter
is the identity on them.  A smooth frame has what a render has: unit normals that turn slowly (then scaled by a random length in
[0.5, 1.5]: the filter normalises), albedo and depth ramps with one depth step, a sky patch (zero normal, depth 0), a patch with no normal at the surface's depth, a converged corner
(variance exactly 0), and a colour that is a smooth base plus per-pixel noise whose level the variance matches.  Everything is
float32, as the device takes it.

The metric is per pixel and per channel: |got - want| / max(|want|, 1e-3), its maximum over the frame.  E32 is that distance between
the statement (tests/denoise_ref.py) evaluated in float32 and in float64; the device is held to BOUND_FACTOR x E32 of its case."""
import functools

import numpy as np

from denoise_ref import denoise

SIGMAS = (2.0, 128.0, 0.1, 0.1)  # jade_denoise_defaults: luminance, normal, depth, albedo
SMOOTH_SIZES = ((23, 37), (40, 7), (16, 16), (1, 1), (1, 19), (19, 1), (15, 17), (48, 64))  # height x width
ITERATIONS = (1, 2, 3, 5, 8)
BOUND_FACTOR = 16.0  # the device's expf / powf are a few ulp where numpy's are one, and an exponent of 128 multiplies them
FLOOR = 1e-3


def smooth(h, w, seed=None):
    """(rgb, variance, albedo, normal, depth) of a smooth h x w frame, float32; the seed defaults to one per size."""
    rng = np.random.default_rng(1000 * h + w if seed is None else seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    n = np.stack([0.3 * np.sin(xx / 7.0), 0.3 * np.cos(yy / 5.0), np.ones_like(xx)], -1)
    n /= np.sqrt((n * n).sum(-1))[..., None]
    n *= 0.5 + rng.random((h, w, 1))
    alb = 0.5 + 0.004 * xx[..., None] + 0.003 * yy[..., None] * np.array([1, 0.5, 0.2])
    dep = 2.0 + 0.01 * xx + 0.02 * yy
    dep[:, w // 2:] += 1.5  # the depth step
    base = 0.6 + 0.3 * np.sin(xx / 9.0)[..., None] * np.array([1, 0.7, 0.4]) + 0.1 * np.cos(yy / 6.0)[..., None]
    sd = 0.02 + 0.2 * rng.random((h, w))
    rgb = base + sd[..., None] * rng.normal(size=(h, w, 3))
    var = sd ** 2 * (0.5 + rng.random((h, w)))
    var[:max(1, h // 4), :max(1, w // 4)] = 0.0  # the converged corner
    sky = (yy >= h - min(4, max(1, h // 3))) & (xx >= w - min(6, max(1, w // 3)))
    n[sky] = 0.0
    dep[sky] = 0.0
    # ... and a 3x3 patch without a normal at the surface's own depth (a caller's image may have one): against the sky w_z is e^-10
    # whatever the depth, which hides what w_n does between a zero normal and a non-zero one
    n[(np.abs(yy - h // 2) <= 1) & (np.abs(xx - (w // 4 + 2)) <= 1)] = 0.0
    return tuple(np.ascontiguousarray(a, np.float32) for a in (rgb, var, alb, n, dep))


def case_name(h, w):
    return f"smooth {h}x{w}"


@functools.lru_cache(maxsize=None)
def case(h, w):
    ins = smooth(h, w)
    for a in ins:
        a.setflags(write=False)
    return ins


def worst(got, want):
    """The metric: the largest |got - want| / max(|want|, FLOOR) over every pixel and channel."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), FLOOR)).max())


def ratio_map(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.maximum(np.abs(want), FLOOR)


_want, _e32 = {}, {}


def _key(ins, iterations, sigmas):
    return (tuple(a.tobytes() for a in ins), tuple(a.shape for a in ins), iterations, tuple(float(s) for s in sigmas))


def want(ins, iterations, sigmas=SIGMAS):
    """The float64 statement's colour for these inputs (computed once, read-only)."""
    k = _key(ins, iterations, sigmas)
    if k not in _want:
        with np.errstate(all="ignore"):
            out = denoise(*ins, iterations, *sigmas)[0]
        out.setflags(write=False)
        _want[k] = out
    return _want[k]


def e32(ins, iterations, sigmas=SIGMAS):
    """E32 of these inputs: the statement in float32 against the statement in float64, by the metric.  Pixels that are not finite in
    the statement (unusable ones) compare by their bits elsewhere and are left out here."""
    k = _key(ins, iterations, sigmas)
    if k not in _e32:
        w = want(ins, iterations, sigmas)
        with np.errstate(all="ignore"):
            got = denoise(*ins, iterations, *sigmas, dtype=np.float32)[0]
        ok = np.isfinite(w)
        _e32[k] = worst(got[ok], w[ok])
    return _e32[k]


def bound(ins, iterations, sigmas=SIGMAS):
    return BOUND_FACTOR * e32(ins, iterations, sigmas)
