"""The denoiser on the MI355X (include/jade_bvh.h: jade_render_guides, jade_render_denoise, jade_denoise_image).

The filter against tests/denoise_ref.py, its exact properties, the guides against tests/jade_spec.py's float64 camera ray and
brute-force hit, the variance against numpy on per-sample values, the consistency of the entry points with each other and with the
render, the quality gain against a disjoint reference, and the error codes."""
import ctypes as C

import numpy as np
import pytest

from conftest import B, counters, config_scene, rel_l2
from jaderaytracerendering_amd import _abi

from adaptive_ref import lane_sums
from denoise_ref import denoise, pixel_variance
from guide_cases import Geometry, spec_guide
from render_helpers import with_params

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _params(name, spp, width=None, height=None, **kw):
    hs, cfg = config_scene(name)
    p = B.params_from_config(cfg, spp=spp, **kw)
    if width:
        p.width, p.height = width, height
    return hs, p


def _dp(hip, **kw):
    d = hip.denoise_defaults()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ref(hip, rgb, var, alb, nrm, dep, d):
    return denoise(rgb, var, alb, nrm, dep, d.iterations, d.sigma_luminance, d.sigma_normal, d.sigma_depth, d.sigma_albedo)[0]


def _synthetic(kind, h, w, seed=0):
    rng = np.random.default_rng(seed)
    rgb = rng.random((h, w, 3)).astype(np.float32) * 2
    var = (rng.random((h, w)) * 0.05).astype(np.float32)
    alb = rng.random((h, w, 3)).astype(np.float32)
    nrm = rng.normal(size=(h, w, 3)).astype(np.float32)
    dep = (rng.random((h, w)) + 0.5).astype(np.float32)
    if kind == "edges":  # step edges in every guide, a sky region (zero normal, depth 0)
        alb[:] = 0.2
        alb[:, w // 3:] = 0.7
        nrm[:] = [0, 0, 1]
        nrm[h // 2:] = [0, 1, 0]
        yy, xx = np.mgrid[0:h, 0:w]
        dep[:] = np.where(xx + yy < (h + w) // 2, 1.0, 3.0)
        nrm[:3, :5] = 0
        dep[:3, :5] = 0
    return rgb, var, alb, nrm, dep


# ------------------------------------------------------------------------------------------------------------- filter --

@pytest.mark.parametrize("kind,h,w", [("random", 17, 24), ("edges", 20, 33), ("random", 40, 7)])
@pytest.mark.parametrize("iterations", [1, 3, 8])
def test_filter_matches_the_reference(hip, kind, h, w, iterations):
    ins = _synthetic(kind, h, w)
    d = _dp(hip, iterations=iterations)
    got = hip.denoise_image(*ins, params=d)
    assert rel_l2(got, _ref(hip, *ins, d)) <= TOL


def test_filter_matches_the_reference_on_a_real_frame(hip):
    hs, p = _params("C1", 16, 64, 48)
    with hip.scene(hs) as sc:
        sc.begin(p)
        sc.step(16)
        g = sc.guides(4)
        rgb, _ = sc.resolve(want_bgr8=False)
    d = _dp(hip)
    got = hip.denoise_image(rgb, g["variance"], g["albedo"], g["normal"], g["depth"], params=d)
    assert np.isfinite(got).all()
    assert rel_l2(got, _ref(hip, rgb, g["variance"], g["albedo"], g["normal"], g["depth"], d)) <= TOL


def test_zero_iterations_is_resolve_for_both_tone_operators(hip):
    hs, p = _params("tinyjade", 16, 40, 24)
    with hip.scene(hs) as sc:
        sc.begin(p)
        sc.step(16)
        for tm, limit in ((_abi.TONEMAP_ACES, 0.0), (_abi.TONEMAP_REINHARD, 1.5)):
            r0, b0 = sc.resolve(tonemap=tm, limit=limit)
            r1, b1 = sc.denoise(_dp(hip, iterations=0), tonemap=tm, limit=limit)
            assert np.array_equal(r0.view(np.uint32), r1.view(np.uint32))
            assert np.array_equal(b0, b1)


def test_opposite_normals_keep_the_halves_apart(hip):
    h, w = 24, 32
    rgb, var, alb, nrm, dep = _synthetic("random", h, w, 5)
    alb[:] = 0.5
    dep[:] = 1.0
    nrm[:] = [0, 0, 1]
    nrm[:, w // 2:] = [0, 0, -1]
    d = _dp(hip, iterations=1)
    a = hip.denoise_image(rgb, var, alb, nrm, dep, params=d)
    rgb2 = rgb.copy()
    rgb2[:, w // 2:] *= 7.0
    b = hip.denoise_image(rgb2, var, alb, nrm, dep, params=d)
    assert np.array_equal(a[:, :w // 2].view(np.uint32), b[:, :w // 2].view(np.uint32))


def test_constant_colour_stays_constant(hip):
    h, w = 30, 41
    _, var, alb, nrm, dep = _synthetic("edges", h, w, 6)
    rgb = np.broadcast_to(np.float32([0.3, 0.8, 0.05]), (h, w, 3)).copy()
    got = hip.denoise_image(rgb, var, alb, nrm, dep, params=_dp(hip, iterations=5))
    np.testing.assert_allclose(got, rgb, rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------- guides --

@pytest.mark.parametrize("name,w,h", [("tinyjade", 24, 16), ("C1", 12, 10)])
def test_guides_match_the_spec(hip, name, w, h):
    hs, p = _params(name, 4, w, h)
    S = Geometry(hs)
    with hip.scene(hs) as sc:
        sc.begin(p)
        sc.step(4)
        g = sc.guides(1)
    ok = 0
    for y in range(h):
        for x in range(w):
            a, n, z = spec_guide(S, x, y, p, p.frame)
            good = (np.allclose(g["albedo"][y, x], a, rtol=0, atol=1e-6) and np.allclose(g["normal"][y, x], n, rtol=0, atol=1e-6)
                    and abs(g["depth"][y, x] - z) <= 1e-5 * max(1.0, abs(z)))
            ok += bool(good)
    assert ok >= 0.99 * w * h, f"{ok} of {w * h} pixels agree with the spec"


def test_guides_average_their_samples_in_order(hip):
    hs, p = _params("C1", 4, 40, 24, frame=7)
    with hip.scene(hs) as sc:
        sc.begin(p)
        sc.step(4)
        g4 = sc.guides(4)
        ones = []
        for s in range(4):
            sc.begin(with_params(p, frame=7 + s))
            sc.step(4)
            ones.append(sc.guides(1))
    for k in ("albedo", "normal", "depth"):
        acc = np.zeros_like(g4[k])
        for s in range(4):
            acc = (acc + ones[s][k]).astype(np.float32)
        want = (acc * np.float32(0.25)).astype(np.float32)
        assert np.array_equal(g4[k].view(np.uint32), want.view(np.uint32)), k


# ----------------------------------------------------------------------------------------------------------- variance --

def _samples(sc, p, n):
    return np.stack([sc.render(with_params(p, spp=1, frame=s), want_bgr8=False)[0] for s in range(n)])


@pytest.mark.parametrize("n", [2, 16, 2048])
def test_variance_matches_numpy(hip, n):
    hs, p = _params("tinyjade", n, 16, 16) if n > 16 else _params("tinyjade", n, 37, 21)
    with hip.scene(hs) as sc:
        x = _samples(sc, p, n)
        sc.begin(with_params(p, spp=n))
        sc.step(n)
        got = sc.guides(1)["variance"]
    want = pixel_variance(lane_sums(x), n)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-12)


def test_variance_is_nan_where_not_estimable(hip):
    hs, p = _params("tinyjade", 1, 16, 16)
    with hip.scene(hs) as sc:
        sc.begin(p)
        sc.step(1)
        assert np.isnan(sc.guides(1)["variance"]).all()
        sc.step(1024)  # 1025 samples: above the lane count and not a multiple of it
        assert np.isnan(sc.guides(1)["variance"]).all()


# -------------------------------------------------------------------------------------------------------- consistency --

def test_render_denoise_is_denoise_image_on_the_exported_inputs(hip):
    hs, p = _params("C1", 16, 50, 36)
    d = _dp(hip)
    with hip.scene(hs) as sc:
        sc.begin(p)
        sc.step(16)
        r1, b1 = sc.denoise(d)
        r2, b2 = sc.denoise(d)
        assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32)) and np.array_equal(b1, b2)  # two calls, same bits
        g = sc.guides(d.guide_spp)
        rgb, _ = sc.resolve(want_bgr8=False)
    got = hip.denoise_image(rgb, g["variance"], g["albedo"], g["normal"], g["depth"], params=d)
    assert np.array_equal(got.view(np.uint32), r1.view(np.uint32))


def test_two_rank_guides_assembled_equal_the_one_rank_denoise(hip):
    hs, p = _params("C1", 16, 50, 36)
    d = _dp(hip)
    with hip.scene(hs) as sc:
        sc.begin(p)
        sc.step(16)
        want, _ = sc.denoise(d, want_bgr8=False)
    rgb = np.zeros((p.height, p.width, 3), np.float32)
    g = {k: np.zeros_like(v) for k, v in {"albedo": rgb, "normal": rgb, "depth": rgb[..., 0], "variance": rgb[..., 0]}.items()}
    for r in range(2):
        q = with_params(p, tile_rank=r, tile_nranks=2)
        with hip.scene(hs) as sc:
            sc.begin(q)
            sc.step(16)
            gr = sc.guides(d.guide_spp)
            owned = ~np.isnan(gr["depth"])
            rr, _ = sc.resolve(want_bgr8=False)
            with pytest.raises(B.JadeError) as e:
                sc.denoise(d)
            assert e.value.code == _abi.JADE_ERR_UNSUPPORTED
        rgb[owned] = rr[owned]
        for k in g:
            g[k][owned] = gr[k][owned]
    got = hip.denoise_image(rgb, g["variance"], g["albedo"], g["normal"], g["depth"], params=d)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_denoise_between_steps_changes_nothing(hip):
    hs, p = _params("C1", 32, 64, 48)
    with hip.scene(hs) as sc:
        sc.begin(p)
        st = sc.step(32)
        sc.flush(st)
        r0, b0 = sc.resolve()
        sc.begin(p)
        s1 = sc.step(16)
        sc.denoise()
        sc.guides(4)
        s2 = sc.step(16)
        sc.flush(s2)
        r1, b1 = sc.resolve()
    assert np.array_equal(r0.view(np.uint32), r1.view(np.uint32)) and np.array_equal(b0, b1)
    c1, c2 = counters(s1), counters(s2)
    assert counters(st) == {k: c1[k] + c2[k] for k in c1}


def test_denoise_after_adaptive_uses_each_tiles_count(hip):
    hs, p = _params("C1", 64, 64, 48)
    d = _dp(hip)
    with hip.scene(hs) as sc:
        _, _, tile_spp, _ = sc.render_adaptive(p, 4, 0.05)
        got, _ = sc.denoise(d, want_bgr8=False)
        g = sc.guides(d.guide_spp)
        rgb, _ = sc.resolve(want_bgr8=False)
    assert len(np.unique(tile_spp)) > 1, "the test wants tiles that stopped at different counts"
    want = hip.denoise_image(rgb, g["variance"], g["albedo"], g["normal"], g["depth"], params=d)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_result_does_not_depend_on_records_per_pixel(hip):
    hs, p = _params("C1", 16, 64, 48)
    out, rpp = [], []
    for msb in (0, 1 << 21):
        with hip.scene(hs) as sc:
            sc.begin(with_params(p, max_state_bytes=msb))
            rpp.append(sc.query(_abi.Q_RECORDS_PER_PIXEL))
            sc.step(16)
            out.append(sc.denoise()[0])
    assert rpp[0] != rpp[1]
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ quality --

def _rel_mse(x, r):
    x = x.astype(np.float64)
    r = r.astype(np.float64)
    return float(np.mean((x - r) ** 2 / (r * r + 1e-2)))


@pytest.mark.parametrize("name,w,h,spp", [("C1", None, None, 16), ("C2", 512, 512, 32)])
def test_denoised_frame_halves_the_error(hip, name, w, h, spp):
    hs, p = _params(name, spp, w, h, walk=_abi.WALK_EARLY_EXIT)
    with hip.scene(hs) as sc:
        ref, _, _ = sc.render(with_params(p, spp=4096, frame=1 << 20), want_bgr8=False)
        sc.begin(p)
        sc.step(spp)
        noisy, _ = sc.resolve(want_bgr8=False)
        den, _ = sc.denoise(want_bgr8=False)
    e0, e1 = _rel_mse(noisy, ref), _rel_mse(den, ref)
    print(f"{name} {spp} spp: relMSE noisy {e0:.4g}, denoised {e1:.4g} ({e1 / e0:.3f} x)")
    assert e1 <= 0.5 * e0, (e0, e1)


# ------------------------------------------------------------------------------------------------------------- errors --

def test_error_codes(hip):
    hs, p = _params("tinyjade", 4, 32, 32)
    img = _synthetic("random", 8, 8)
    for bad in (dict(iterations=-1), dict(iterations=9), dict(guide_spp=0), dict(guide_spp=65), dict(sigma_luminance=0.0),
                dict(sigma_luminance=float("nan")), dict(sigma_normal=-1.0), dict(sigma_depth=0.0), dict(sigma_albedo=float("nan"))):
        with pytest.raises(B.JadeError) as e:
            hip.denoise_image(*img, params=_dp(hip, **bad))
        assert e.value.code == _abi.JADE_ERR_INVALID, bad
    with hip.scene(hs) as sc:
        fg, fd = sc.backend.hip_only("jade_render_guides"), sc.backend.hip_only("jade_render_denoise")
        z = np.zeros(32 * 32 * 3, np.float32)
        assert fg(sc._h, 1, z.ctypes.data, None, None, None) == _abi.JADE_ERR_INVALID  # no render begun
        d = _dp(hip)
        assert fd(sc._h, C.byref(d), 0, 0.0, z.ctypes.data, None) == _abi.JADE_ERR_INVALID
        sc.begin(p)
        sc.step(1)
        with pytest.raises(B.JadeError) as e:
            sc.denoise()  # n = 1: no variance
        assert e.value.code == _abi.JADE_ERR_INVALID
        sc.step(3)
        for bad in (dict(iterations=9), dict(sigma_depth=float("nan"))):
            with pytest.raises(B.JadeError) as e:
                sc.denoise(_dp(hip, **bad))
            assert e.value.code == _abi.JADE_ERR_INVALID
        with pytest.raises(B.JadeError) as e:
            sc.guides(0)
        assert e.value.code == _abi.JADE_ERR_INVALID
        sc.begin(with_params(p, tile_nranks=2))
        sc.step(4)
        with pytest.raises(B.JadeError) as e:
            sc.denoise()
        assert e.value.code == _abi.JADE_ERR_UNSUPPORTED
