"""The draw of JADE_ENV_IMPORTANCE on the device (env_sample, jade_shade.h, through libjade_hip_debug.so's jade_debug_env_sample) against
the float64 statement tests/env_importance_spec.py, uniform row by uniform row, on the maps of tests/test_env_importance_cpu.py: the
texel and the own / alias decision are equal, the direction and the ratio lie within a bound DERIVED from the fp32 evaluation, the
ratio is never negative, and the wrapper the shading kernel calls makes exactly four draws in the stated order.

The bound on a direction component (include/jade_rt.h states the fp32 evaluation):
  * theta = fl(fl(PI) * fl(fl(j + u4) / H)) and phi = fl(fl(2 PI) * fl(fl(fl(i + u3) / W) - 0.5)) carry at most three fp32 roundings
    (the subtraction is exact for u >= 0.25 and half a rounding below) of magnitudes up to 2 PI:     A = 3 * 2^-24 * 2 PI = 1.124e-6;
  * jade_sincosf is within S = 2.5e-7 of sin and cos (tests/test_fpmath.py::test_sincos_accuracy's bound, absolute);
  * a component is a product of two such values, each <= 1, rounded once:                           D = 2 (A + S) + 2^-24 = 2.81e-6.
The bound on the ratio, absolute because sin(theta) vanishes at the poles: (PI / q) * D + 4 * 2^-24 * ratio (the sine's error, then
the roundings of the product, of the quotient and of the table's fp32 q)."""
import numpy as np
import pytest

import env_importance_spec as spec
import env_spec

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
ANGLE_BOUND = 3 * EPS * 2 * spec.PI
SINCOS_BOUND = 2.5e-7
DIR_BOUND = 2 * (ANGLE_BOUND + SINCOS_BOUND) + EPS

CASES = [(w, h, kind) for (w, h) in spec.MAP_SIZES for kind in spec.KINDS]
ONE = np.float32(1.0)
BELOW_ONE = np.nextafter(ONE, np.float32(0))  # 1 - 2^-24


def uniform_rows(table, w, h):
    """float32 [n, 4]: the rows a map is tried on (30 k + 31 N: 30 036 for 1x1, 93 493 for 64x32)."""
    n = w * h
    rng = np.random.default_rng(17 * w + h)
    f32 = np.float32
    rows = [rng.random((30000, 4), dtype=np.float32)]
    mid = ((np.arange(n) + 0.5) / n).astype(f32)          # one u1 per slot
    rows.append(np.column_stack([mid, rng.random((n, 3), dtype=np.float32)]))
    # u1 at 0, at 1.0f and at k / N with both neighbours
    k = (np.arange(n + 1) / n).astype(f32)
    u1 = np.unique(np.clip(np.concatenate([k, np.nextafter(k, f32(-1)), np.nextafter(k, f32(2)), [f32(0), ONE]]), 0, 1).astype(f32))
    rows.append(np.column_stack([u1, rng.random((len(u1), 3), dtype=np.float32)]))
    for u2 in (f32(0), ONE):  # ... and the two ends once more with the own and the alias texel: u1 = 1.0f is the last slot's, not the first's
        rows.append(np.column_stack([np.array([0, ONE], f32), np.full(2, u2), rng.random((2, 2), dtype=np.float32)]))
    # u2 at accept and one ulp to either side, for every slot
    acc = table["accept"][spec.slot_of(mid, n)]
    for u2 in (acc, np.nextafter(acc, f32(-1)), np.nextafter(acc, f32(2))):
        rows.append(np.column_stack([mid, np.clip(u2, 0, 1).astype(f32), rng.random((n, 2), dtype=np.float32)]))
    # u3, u4 at 0, 1.0f and 1 - 2^-24 for the own and the alias texel of every slot: the seam column and both pole rows among them
    edge = np.array([0.0, ONE, BELOW_ONE], f32)
    for u2 in (f32(0), ONE):
        for u3 in edge:
            for u4 in edge:
                rows.append(np.column_stack([mid, np.full(n, u2), np.full(n, u3), np.full(n, u4)]))
    # ... and crossed with a random partner
    for col in (2, 3):
        for val in edge:
            r = rng.random((n, 4), dtype=np.float32)
            r[:, 0], r[:, col] = mid, val
            rows.append(r)
    return np.ascontiguousarray(np.concatenate(rows), f32)


@pytest.fixture(scope="module", params=CASES, ids=[f"{w}x{h}-{k}" for w, h, k in CASES])
def case(request, hip_debug):
    """(scene handle, table, W, H, uniforms, what the statement draws, what the device draws) - computed once per map."""
    w, h, kind = request.param
    env = spec.make_map(w, h, kind)
    table = spec.table_of(hip_debug.lib, env)
    u = uniform_rows(table, w, h)
    want = spec.draw(table, w, h, *u.T)
    with hip_debug.scene(env_spec.sky_scene(env)) as sc:
        got = spec.sample_device(sc, u)
        rng_in = np.concatenate([np.arange(1, 4097, dtype=np.uint32) * np.uint32(2654435761), np.uint32([0, 1, 0xffffffff, 0x80000000])])
        got_rng = spec.sample_device_rng(sc, rng_in)
    return dict(w=w, h=h, kind=kind, table=table, u=u, want=want, got=got, rng_in=rng_in, got_rng=got_rng)


def test_texel_and_own_are_the_statements(case):
    texel, own = case["want"][:2]
    _, _, got_texel, got_own = case["got"]
    bad = np.flatnonzero((got_texel != texel) | (got_own != own))
    assert len(bad) == 0, [(case["u"][i].tolist(), int(got_texel[i]), bool(got_own[i]), int(texel[i]), bool(own[i])) for i in bad[:5]]
    n = case["w"] * case["h"]
    assert len(np.unique(texel)) == n, "every texel is drawn (as its slot's own, at u2 = 0)"
    assert len(np.unique(spec.slot_of(case["u"][:, 0], n))) == n, "every slot is drawn"


def test_direction_and_ratio_within_the_derived_bound(case):
    _, _, d, ratio, q = case["want"]
    got_d, got_ratio, _, _ = case["got"]
    assert np.isfinite(got_d).all() and np.isfinite(got_ratio).all()
    err = np.abs(got_d.astype(np.float64) - d)
    rerr = np.abs(got_ratio.astype(np.float64) - ratio)
    rtol = (spec.PI / q) * DIR_BOUND + 4 * EPS * ratio
    print(f"map {case['w']}x{case['h']} {case['kind']}: worst |direction - float64| {err.max():.3g} (bound {DIR_BOUND:.3g}), "
          f"worst ratio error / its bound {(rerr / rtol).max():.3g}")
    i = int(err.max(1).argmax())
    assert err.max() <= DIR_BOUND, (case["u"][i].tolist(), got_d[i].tolist(), d[i].tolist())
    i = int((rerr / rtol).argmax())
    assert (rerr <= rtol).all(), (case["u"][i].tolist(), float(got_ratio[i]), float(ratio[i]), float(rtol[i]))
    assert np.abs((got_d.astype(np.float64) ** 2).sum(1) - 1).max() <= 4 * DIR_BOUND


def test_ratio_is_never_negative(case):
    got_d, got_ratio, _, _ = case["got"]
    assert (got_ratio >= 0).all(), case["u"][got_ratio < 0][:5].tolist()
    assert not np.signbit(got_ratio).any()
    # u4 = 1.0f in the bottom row - theta = fl(PI), the end of the range, where the sine is 1.5e-7 - is among the rows, and points straight down
    texel = case["want"][0]
    low = (texel // case["w"] == case["h"] - 1) & (case["u"][:, 3] == ONE)
    assert low.any()
    assert np.abs(got_d[low] - np.float32([0, -1, 0])).max() <= DIR_BOUND


def test_the_wrapper_makes_the_four_draws_in_order(case):
    """jade_debug_env_sample_rng runs env_sample as bounce_branch calls it: the state it leaves is four Wang steps on, and its result is
    the body's on the four numbers those steps give, u1 first."""
    after, d, ratio = case["got_rng"]
    s = case["rng_in"]
    us = []
    for _ in range(4):
        s = spec.wang(s)
        us.append(spec.uniform_of(s))
    assert np.array_equal(after, s)
    texel, own, want_d, want_ratio, q = spec.draw(case["table"], case["w"], case["h"], *us)
    assert np.abs(d.astype(np.float64) - want_d).max() <= DIR_BOUND
    assert (np.abs(ratio.astype(np.float64) - want_ratio) <= (spec.PI / q) * DIR_BOUND + 4 * EPS * want_ratio).all()


def test_a_map_within_the_cap_renders_and_the_debug_entries_check_their_arguments(hip, hip_debug):
    """The over-large map rule is a predicate on (W, H) alone (tests/test_env_importance_cpu.py tries it at the cap and beyond without a
    33 M-texel upload); here: a small map passes it in jade_render_begin, and the entry points refuse what they cannot run."""
    from jaderaytracerendering_amd import _abi, backend as B
    env = spec.make_map(7, 5, "random")
    hs = env_spec.sky_scene(env)
    p = env_spec.sky_params(env_spec.CAMERA_POSES[0])
    p.env_sampling = _abi.ENV_IMPORTANCE
    with hip.scene(hs) as sc:
        rgb, _, st = sc.render(p)
    assert np.isfinite(rgb).all() and st.samples == p.width * p.height
    import ctypes as C
    with hip_debug.scene(hs) as sc:
        fn = sc.backend.lib.jade_debug_env_sample
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
        u = np.zeros((4, 4), np.float32)
        out = np.zeros(12, np.float32)
        assert fn(sc._h, 0, u.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data) == _abi.JADE_ERR_INVALID
        assert fn(sc._h, 4, None, out.ctypes.data, out.ctypes.data, out.ctypes.data) == _abi.JADE_ERR_INVALID
        assert fn(None, 4, u.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data) == _abi.JADE_ERR_INVALID
