"""jade_despeckle_image on the MI355X against the float32 statement (tests/despeckle_spec.py) on every case of tests/despeckle_cases.py:
colour, variance and scale compared as uint32 words, the report's four counts equal, no tolerance."""
import ctypes as C

import numpy as np
import pytest

from jaderaytracerendering_amd import _abi

import despeckle_cases as K

pytestmark = pytest.mark.gpu


def _params(hip, case):
    p = hip.despeckle_defaults()
    for k, v in case.params.items():
        setattr(p, k, v)
    return p


def _run(hip, case):
    return hip.despeckle_image(K.frame(case.kind, case.w, case.h), K.variance(case.vkind, case.kind, case.w, case.h), _params(hip, case))


@pytest.mark.parametrize("case", K.CASES, ids=[c.id for c in K.CASES])
def test_the_device_gives_the_statements_bits(hip, case):
    got, want = _run(hip, case), K.want(case)
    assert K.same(got, want), K.differences(got, want)


def test_twice_gives_the_same_bits_and_iterations_zero_the_input(hip):
    case = K.IN_PLACE_CASE
    assert K.same(_run(hip, case), _run(hip, case))
    x, v = K.frame("bad", 33, 20), K.variance("negative", "bad", 33, 20)
    p = _params(hip, case)
    p.iterations = 0
    rgb, var, scale, rep = hip.despeckle_image(x, v, p)
    assert np.array_equal(K.bits(rgb), K.bits(x)) and np.array_equal(K.bits(var), K.bits(v)) and (scale == 1.0).all()
    assert rep == K.S.despeckle(x, v, iterations=0)[3]


def test_in_place_through_the_c_entry_point(hip):
    case = K.IN_PLACE_CASE
    want = K.want(case)
    assert want[3]["n_clamped"] > 0 and want[3]["n_established"] > 0
    rgb = K.frame(case.kind, case.w, case.h).copy()
    var = K.variance(case.vkind, case.kind, case.w, case.h).copy()
    scale = np.zeros((case.h, case.w), np.float32)
    rep = _abi.DespeckleReport()
    p = _params(hip, case)
    fn = hip.hip_only("jade_despeckle_image")
    rc = fn(0, case.w, case.h, rgb.ctypes.data, var.ctypes.data, C.byref(p), rgb.ctypes.data, var.ctypes.data, scale.ctypes.data, C.byref(rep))
    assert rc == _abi.JADE_OK, hip.lib.jade_last_error().decode()
    got = (rgb, var, scale, {k: int(getattr(rep, k)) for k in K.S.REPORT})
    assert K.same(got, want), K.differences(got, want)
    # every output but the frame is optional
    out = np.zeros_like(rgb)
    x = K.frame(case.kind, case.w, case.h)
    assert fn(0, case.w, case.h, x.ctypes.data, None, C.byref(p), out.ctypes.data, None, None, None) == _abi.JADE_OK
    assert np.array_equal(K.bits(out), K.bits(K.S.despeckle(x, None, **case.params)[0]))


def test_a_one_pixel_wide_frame_at_the_largest_height(hip):
    """1 x 524280: 65535 blocks in grid.y, every one a column of 8 pixels with a halo that is out of the image left and right.  (One
    row more is refused: tests/test_despeckle_cpu.py.)"""
    case = K.TALL_CASE
    assert (case.w, case.h) == (1, 8 * 65535)
    got, want = _run(hip, case), K.want(case)
    assert want[3]["n_clamped"] > 1000 and want[3]["n_established"] > 1000
    assert K.same(got, want), K.differences(got, want)
