"""Exposure on the MI355X (include/jade_bvh.h: jade_render_meter, jade_render_resolve_exposed, jade_expose_image).

Everything here is bit for bit: the meter is integers (tests/exposure_spec.py states them in numpy), the exposure a host function of
those integers, and the bytes the existing tone pack of one float product."""
import ctypes as C

import numpy as np
import pytest

from conftest import B, counters, config_scene
from jaderaytracerendering_amd import _abi

import exposure_spec as X
from tone_spec import oracle_tone_pack

pytestmark = pytest.mark.gpu

W, H, SPP = 45, 27, 16  # 3 x 2 tiles, the right column and the upper row partial


def _params(**kw):
    hs, cfg = config_scene("tinyjade")
    p = B.params_from_config(cfg, spp=SPP, **kw)
    p.width, p.height = W, H
    return hs, p


def _with(p, **kw):
    q = type(p).from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _display(hip, **kw):
    d = hip.display_defaults()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _same_meter(got, want, what):
    assert np.array_equal(got.bins, want.bins), (what, np.flatnonzero(got.bins != want.bins)[:8])
    assert (got.n_zero, got.n_negative, got.n_nonfinite) == (want.n_zero, want.n_negative, want.n_nonfinite), what
    assert got.lum_min.tobytes() == want.lum_min.tobytes() and got.lum_max.tobytes() == want.lum_max.tobytes(), (what, got, want)
    assert got == want


@pytest.fixture(scope="module")
def render(hip):
    """tinyjade, 45 x 27, 16 spp, left in progress on its scene: (scene, params, jade_render_resolve_ex's rgb and bgr8 for ACES)."""
    hs, p = _params()
    with hip.scene(hs) as sc:
        sc.begin(p)
        sc.step(SPP)
        rgb, bgr = sc.resolve(tonemap=_abi.TONEMAP_ACES)
        yield sc, p, rgb, bgr


# ------------------------------------------------------------------------------------------------- crafted pixels --

def _crafted():
    """[n, 3] float32: the inputs the meter's arithmetic can get wrong."""
    rng = np.random.default_rng(5)
    edges = B.Meter.bin_edges().astype(np.float32)  # 513 values, the last one 2^32: all exact in float32
    near = np.concatenate([np.nextafter(edges, np.float32(0)), edges, np.nextafter(edges, np.float32(np.inf))])
    grey = np.repeat(near.reshape(-1, 1), 3, 1)
    sub = np.float32([1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 2.0 ** -33, 2.0 ** -32, 2.0 ** 32, 3.0e38, 3.4028235e38, 0.0, -0.0])
    special = [np.repeat(sub.reshape(-1, 1), 3, 1), np.float32([(-1, -1, -1), (-1e-45, 0, 0), (1, -1, 1), (5, -0.5, -20.000002), (-3e38, 0, 0),
                                                               (3.4028235e38, 3.4028235e38, 3.4028235e38), (0.0, -0.0, 0.0)])]
    for bad in (np.nan, np.inf, -np.inf):
        for ch in range(3):
            row = np.float32([0.5, 0.25, 2.0])
            row[ch] = bad
            special.append(row.reshape(1, 3))
    special.append(np.float32([(np.inf, -np.inf, 1.0), (np.nan, np.nan, np.nan)]))
    # coloured triples whose double sum lies within a few ulps of an edge, on both sides of it
    c = rng.random((6000, 3)) + 0.01
    target = np.float64(edges[rng.integers(1, 512, 6000)])
    s = 0.3 * c[:, 0] + 0.6 * c[:, 1] + 0.1 * c[:, 2]
    coloured = (c * (target / s)[:, None] * (1.0 + rng.integers(-3, 4, 6000)[:, None] * 2.0 ** -24)).astype(np.float32)
    # 50 000 random colours over 70 decades
    rnd = (rng.random((50000, 3)) * 10.0 ** rng.uniform(-35, 35, (50000, 1))).astype(np.float32)
    return np.concatenate([grey, *special, coloured, rnd]).astype(np.float32)


@pytest.fixture(scope="module")
def crafted():
    px = _crafted()
    y, cls, b = X.classify(px)
    assert len(np.unique(b[cls == X.POSITIVE])) == X.BINS and all((cls == k).sum() > 3 for k in range(4))  # the inputs reach everything
    return px


def _frames(crafted):
    rng = np.random.default_rng(6)
    n = len(crafted)
    yield "all crafted pixels", crafted.reshape(1, n, 3)
    yield "1 x 1", crafted[700:701].reshape(1, 1, 3)
    yield "1 x 1 NaN", np.float32([[[np.nan, 0, 0]]])
    yield "17 x 5", crafted[rng.integers(0, n, 85)].reshape(5, 17, 3)
    yield "257 x 3", crafted[rng.integers(0, n, 771)].reshape(3, 257, 3)
    # one value everywhere: every lane of every wave hits one bin, its count passes 2^16 and 274 blocks' rows are added
    yield "350 x 200 constant", np.broadcast_to(np.float32([0.7, 0.7, 0.7]), (200, 350, 3))
    yield "350 x 200 black", np.zeros((200, 350, 3), np.float32)
    yield "350 x 200 random", crafted[rng.integers(0, n, 70000)].reshape(200, 350, 3)
    # more pixels than the bounded grid has threads (1024 blocks x 256): the grid strides
    yield "521 x 515 random", crafted[rng.integers(0, n, 521 * 515)].reshape(515, 521, 3)


def test_meter_of_crafted_pixels_equals_the_spec(hip, crafted):
    for what, frame in _frames(crafted):
        bgr, e, m = hip.expose_image(frame, want_bgr8=False)
        want = X.meter(frame)
        assert bgr is None and e == 1.0
        assert m.total == frame.shape[0] * frame.shape[1], what
        _same_meter(m, want, what)
    assert m.n_positive > (1 << 16)


def test_expose_image_bytes_equal_the_oracles_tone_pack(hip, oracle, crafted):
    """The plain-image form of k_expose_pack on the crafted pixels (NaN, infinities, negatives, huge values): the oracle's
    bytes of float32(rgb) * float32(e), for a manual and for the automatic exposure."""
    frame = crafted[:20000].reshape(100, 200, 3)
    for tonemap, limit in ((_abi.TONEMAP_ACES, 0.0), (_abi.TONEMAP_REINHARD, 1.5)):
        for mode, e_in in ((_abi.EXPOSURE_MANUAL, 0.37), (_abi.EXPOSURE_AUTO, 1.0)):
            d = _display(hip, tonemap=tonemap, limit=limit, exposure_mode=mode, exposure=e_in)
            bgr, e, m = hip.expose_image(frame, d)
            assert e == hip.meter_exposure(m, d)
            with np.errstate(all="ignore"):
                want = oracle_tone_pack(oracle, frame.reshape(-1, 3) * np.float32(e), tonemap, limit)
            assert np.array_equal(bgr.reshape(-1, 3), want), (tonemap, mode)


# ------------------------------------------------------------------------------------------------- on a render --

@pytest.mark.parametrize("tonemap,limit", [(_abi.TONEMAP_ACES, 0.0), (_abi.TONEMAP_REINHARD, 1.5)])
def test_manual_exposure_one_is_resolve_ex(render, tonemap, limit):
    sc, p, _, _ = render
    rgb0, bgr0 = sc.resolve(tonemap=tonemap, limit=limit)
    rgb, bgr, e, _ = sc.resolve(tonemap=tonemap, limit=limit, exposure=1.0)
    assert e == 1.0
    assert np.array_equal(rgb.view(np.uint32), rgb0.view(np.uint32))
    assert np.array_equal(bgr, bgr0)
    assert bgr.any()


@pytest.mark.parametrize("e", [2.0 ** -3, 0.37, 5.0])
def test_manual_exposures_equal_the_oracles_tone_pack_of_the_product(render, oracle, e):
    sc, p, rgb0, _ = render
    for tonemap, limit in ((_abi.TONEMAP_ACES, 0.0), (_abi.TONEMAP_REINHARD, 1.5)):
        rgb, bgr, used, _ = sc.resolve(tonemap=tonemap, limit=limit, exposure=e)
        assert used == float(np.float32(e))
        assert np.array_equal(rgb.view(np.uint32), rgb0.view(np.uint32))  # never scaled
        want = oracle_tone_pack(oracle, rgb0.reshape(-1, 3) * np.float32(e), tonemap, limit)
        assert np.array_equal(bgr.reshape(-1, 3), want), tonemap


def test_scene_meter_counts_the_image_and_equals_the_spec(hip, render):
    sc, p, rgb0, _ = render
    m = sc.meter()
    assert m.total == W * H  # out-of-image pixels of the edge tiles (k_resolve writes them as 0) are not counted
    _same_meter(m, hip.expose_image(rgb0, want_bgr8=False)[2], "expose_image(out_rgb)")
    _same_meter(m, X.meter(rgb0), "spec")
    assert m.n_positive > 0


def test_auto_exposure(hip, render):
    sc, p, rgb0, bgr0 = render
    d = _display(hip, exposure_mode=_abi.EXPOSURE_AUTO)
    rgb, bgr, e, m = sc.resolve(exposure=d)
    assert e == hip.meter_exposure(m, d)
    assert abs(e - float(X.exposure(m.bins))) <= X.POLICY_RTOL * e
    _same_meter(m, X.meter(rgb0), "spec")
    assert np.array_equal(rgb.view(np.uint32), rgb0.view(np.uint32))
    assert np.array_equal(bgr, sc.resolve(exposure=e)[1])
    assert e != 1.0 and not np.array_equal(bgr, bgr0)
    assert sc.resolve(exposure="auto")[2] == e  # the string form is the defaults' policy
    # another key, another window
    d2 = _display(hip, exposure_mode=_abi.EXPOSURE_AUTO, key=0.5, p_lo=0.0, p_hi=0.5, tonemap=_abi.TONEMAP_REINHARD)
    _, bgr2, e2, m2 = sc.resolve(exposure=d2)
    assert e2 == hip.meter_exposure(m2, d2) and e2 != e
    assert np.array_equal(bgr2, sc.resolve(tonemap=_abi.TONEMAP_REINHARD, limit=d2.limit, exposure=e2)[1])


def test_three_ranks_meters_add_and_their_manual_frames_assemble(hip, render):
    sc, p, rgb0, _ = render
    d = _display(hip, exposure_mode=_abi.EXPOSURE_AUTO)
    _, want_bgr, want_e, want_m = sc.resolve(exposure=d)
    hs, _ = _params()
    scenes, meters = [], []
    try:
        for r in range(3):
            s = hip.scene(hs)
            scenes.append(s)
            s.begin(_with(p, tile_rank=r, tile_nranks=3))
            s.step(SPP)
            meters.append(s.meter())
        total = meters[0] + meters[1] + meters[2]
        _same_meter(total, want_m, "sum of three ranks")
        assert all(m.total > 0 for m in meters) and sum(m.total for m in meters) == W * H
        e = hip.meter_exposure(total, d)
        assert e == want_e
        frame = np.zeros((H, W, 3), np.uint8)
        rgb = np.zeros((H, W, 3), np.float32)
        for s in scenes:
            r_rgb, r_bgr, used, _ = s.resolve(exposure=e)
            assert used == e
            frame |= r_bgr  # (pixels a rank does not own stay 0 in its arrays)
            rgb.view(np.uint32)[...] |= r_rgb.view(np.uint32)
        assert np.array_equal(rgb.view(np.uint32), rgb0.view(np.uint32))
        assert np.array_equal(frame, want_bgr)
    finally:
        for s in scenes:
            s.close()


def test_meter_after_adaptive_uses_each_tiles_count(hip):
    hs, p = _params()
    with hip.scene(hs) as sc:
        rgb, _, tile_spp, _ = sc.render_adaptive(p, 4, 0.1)
        m = sc.meter()
        _, bgr, e, m2 = sc.resolve(exposure="auto")
        manual = sc.resolve(exposure=e)[1]
    print("tile_spp:", tile_spp.tolist())
    _same_meter(m, X.meter(rgb), "spec on the adaptive render's out_rgb")
    _same_meter(m2, m, "resolve's meter")
    assert m.total == W * H and np.array_equal(bgr, manual)


def test_metering_between_steps_changes_nothing(hip, render):
    _, p, rgb0, bgr0 = render
    hs, _ = _params()
    with hip.scene(hs) as sc:
        sc.begin(p)
        st = sc.step(16)
        sc.flush(st)
        sc.begin(p)
        s1 = sc.step(8)
        sc.meter()
        sc.resolve(exposure="auto")
        sc.resolve(exposure=2.0)
        s2 = sc.step(8)
        sc.flush(s2)
        r1, b1 = sc.resolve()
    assert np.array_equal(rgb0.view(np.uint32), r1.view(np.uint32)) and np.array_equal(bgr0, b1)
    c1, c2 = counters(s1), counters(s2)
    assert counters(st) == {k: c1[k] + c2[k] for k in c1}


BAD = (dict(exposure_mode=2), dict(exposure_mode=-1), dict(exposure=0.0), dict(exposure=-2.0), dict(exposure=float("nan")),
       dict(exposure_mode=1, p_lo=0.5, p_hi=0.5), dict(exposure_mode=1, p_lo=0.9, p_hi=0.1), dict(exposure_mode=1, key=0.0),
       dict(exposure_mode=1, min_exposure=0.0), dict(tonemap=7))


def test_bad_arguments(hip, render):
    _, p, rgb0, bgr0 = render
    hs, _ = _params()
    meter_fn, exposed_fn = hip.hip_only("jade_render_meter"), hip.hip_only("jade_render_resolve_exposed")
    image_fn = hip.hip_only("jade_expose_image")
    ok = hip.display_defaults()
    m = _abi.MeterStruct()
    out = np.zeros((H, W, 3), np.uint8)
    with hip.scene(hs) as sc:
        assert meter_fn(sc._h, C.byref(m)) == _abi.JADE_ERR_INVALID  # before begin
        assert exposed_fn(sc._h, C.byref(ok), None, out.ctypes.data, None, None) == _abi.JADE_ERR_INVALID
        sc.begin(p)
        assert meter_fn(sc._h, C.byref(m)) == _abi.JADE_ERR_INVALID  # no sample rendered
        assert exposed_fn(sc._h, C.byref(ok), None, out.ctypes.data, None, None) == _abi.JADE_ERR_INVALID
        sc.step(SPP)
        assert meter_fn(sc._h, None) == _abi.JADE_ERR_INVALID
        assert exposed_fn(sc._h, None, None, out.ctypes.data, None, None) == _abi.JADE_ERR_INVALID  # null parameters
        assert "null" in hip.lib.jade_last_error().decode()
        for bad in BAD:
            with pytest.raises(B.JadeError) as e:
                sc.resolve(exposure=_display(hip, **bad))
            assert e.value.code == _abi.JADE_ERR_INVALID, bad
        with pytest.raises(B.JadeError) as e:
            sc.resolve(exposure=0.0)
        assert e.value.code == _abi.JADE_ERR_INVALID
        assert not out.any()
        rgb, bgr = sc.resolve()  # the scene renders on as if nothing had been asked
        assert np.array_equal(rgb.view(np.uint32), rgb0.view(np.uint32)) and np.array_equal(bgr, bgr0)
        assert np.array_equal(sc.resolve(exposure=1.0)[1], bgr0)
    img = np.ones((4, 5, 3), np.float32)
    for bad in BAD:
        with pytest.raises(B.JadeError) as e:
            hip.expose_image(img, _display(hip, **bad))
        assert e.value.code == _abi.JADE_ERR_INVALID, bad
    assert image_fn(0, 5, 4, img.ctypes.data, None, None, None, None) == _abi.JADE_ERR_INVALID
    assert image_fn(0, 5, 4, None, C.byref(ok), None, None, None) == _abi.JADE_ERR_INVALID
    assert image_fn(0, 0, 4, img.ctypes.data, C.byref(ok), None, None, None) == _abi.JADE_ERR_INVALID
    assert image_fn(0, 5, -1, img.ctypes.data, C.byref(ok), None, None, None) == _abi.JADE_ERR_INVALID
    assert image_fn(10 ** 6, 5, 4, img.ctypes.data, C.byref(ok), None, None, None) == _abi.JADE_ERR_INVALID
    assert image_fn(0, 5, 4, img.ctypes.data, C.byref(ok), None, None, None) == _abi.JADE_OK  # nothing asked for, nothing done
