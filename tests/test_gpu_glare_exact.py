"""Glare on the MI355X, bit for bit: jade_glare_image against the float32 statement of tests/glare_ref.py on the cases of
tests/glare_cases.py.  include/jade_bvh.h fixes every operation and its order, the library is built with -ffp-contract=off
-fno-fast-math, and the kernels have no atomics and one writer per word: there is no tolerance here, every pixel is compared as
three uint32.  tests/test_glare_cpu.py shows what the relative L2 of tests/test_gpu_glare.py lets through instead."""
import ctypes as C

import numpy as np
import pytest

from conftest import B, config_scene
from jaderaytracerendering_amd import _abi

import glare_cases as K

pytestmark = pytest.mark.gpu


def _gp(hip, case):
    p = hip.glare_defaults()
    p.levels, p.strength, p.falloff = case.levels, case.strength, case.falloff
    assert p.falloff == case.falloff  # the cases hold floats already; the strength is rounded here, as the statement rounds it
    return p


def _assert_same_bits(got, case):
    want = K.want(case)
    n, first = K.differences(got, want)
    if n:
        print(f"{case.id}: {n} of {case.w * case.h} pixels differ; (x, y, device bits, statement bits):")
        for d in first:
            print("  ", d)
    assert n == 0, f"{case.id}: {n} pixels differ from the float32 statement, the first at {first[0][:2]}"
    x = K.frame(case.kind, case.w, case.h)
    bad = K.bad_mask(x)
    assert np.array_equal(K.bits(got)[bad], K.bits(x)[bad])  # what the header says of them, whatever the statement does


@pytest.mark.parametrize("case", K.CASES, ids=[c.id for c in K.CASES])
def test_the_device_equals_the_float32_statement_in_every_bit(hip, case):
    _assert_same_bits(hip.glare_image(K.frame(case.kind, case.w, case.h), _gp(hip, case)), case)


@pytest.mark.parametrize("kind,w,h", K.OPERATOR_FRAMES, ids=[f"{k}-{w}x{h}" for k, w, h in K.OPERATOR_FRAMES])
def test_expand_of_reduce_alone(hip, kind, w, h):
    """levels 1, strength 1: the one weight is 1 and (1 - s) is 0, so the output is EXPAND(REDUCE(c)) (0 c + 1 E, both exact but for
    the sign of a zero): k_gl_reduce and gl_expand and nothing else"""
    case = K.operator_case(kind, w, h, 1)
    _assert_same_bits(hip.glare_image(K.frame(kind, w, h), _gp(hip, case)), case)


@pytest.mark.parametrize("kind,w,h", K.OPERATOR_FRAMES, ids=[f"{k}-{w}x{h}" for k, w, h in K.OPERATOR_FRAMES])
def test_one_expand_add_on_top(hip, kind, w, h):
    """levels 2, strength 1: what the test above proves plus one k_gl_expand_add with a coarser level, w_1 L_1 + EXPAND(w_2 L_2)"""
    case = K.operator_case(kind, w, h, 2)
    _assert_same_bits(hip.glare_image(K.frame(kind, w, h), _gp(hip, case)), case)


def test_the_tallest_frame(hip):
    """1 x 1048560: k_gl_out and level 1 of k_gl_reduce launch exactly 65535 blocks in grid.y, the most a grid holds; one row more is
    refused (tests/test_glare_cpu.py).  Out of place through the wrapper, then in place through the C entry point."""
    case = K.TALL_CASE
    assert (case.w, case.h, case.levels) == (1, 16 * 65535, 12)
    x = K.frame(case.kind, case.w, case.h)
    p = _gp(hip, case)
    _assert_same_bits(hip.glare_image(x, p), case)  # (the wrapper raises on any code but JADE_OK)
    buf = x.copy()
    assert hip.hip_only("jade_glare_image")(0, case.w, case.h, buf.ctypes.data, C.byref(p), buf.ctypes.data) == _abi.JADE_OK
    _assert_same_bits(buf, case)


def test_render_glare_at_falloff_2_and_strength_1_is_glare_image_of_the_resolved_frame(hip):
    """The render path through the falloff > 1 branch of the weights and with (1 - s) = 0; tests/test_gpu_glare.py proves the rest
    of jade_render_glare on this 45 x 27 render."""
    hs, cfg = config_scene("tinyjade")
    rp = B.params_from_config(cfg, spp=16)
    rp.width, rp.height = 45, 27
    gp = hip.glare_defaults()
    gp.levels, gp.strength, gp.falloff = 4, 1.0, 2.0
    with hip.scene(hs) as sc:
        sc.begin(rp)
        sc.step(16)
        rgb0, _ = sc.resolve(tonemap=_abi.TONEMAP_ACES)
        rgb, _, _ = sc.glare(gp)
    want = hip.glare_image(rgb0, gp)
    assert not np.array_equal(K.bits(want), K.bits(rgb0))
    n, first = K.differences(rgb, want)
    assert n == 0, (n, first)
    with np.errstate(all="ignore"):
        stated = K.G.glare(rgb0, 4, 1.0, 2.0, np.float32)
    n, first = K.differences(rgb, stated)
    assert n == 0, (n, first)
