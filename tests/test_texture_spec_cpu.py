"""tests/texture_spec.py against the properties "The surface colour, stated" (include/jade_bvh.h) claims for its fetch and its lookup:
no device is involved - these hold the statement itself, which tests/test_gpu_texture.py then holds the device to."""
import numpy as np

import texture_spec as spec

F32 = np.float32
E = 2.0 ** -24


def images():
    rng = np.random.default_rng(7)
    return [rng.uniform(-0.5, 2.0, s).astype(F32) for s in ((4, 8, 3), (16, 16, 3), (5, 7, 3), (1, 1, 3), (32, 3, 3))]


def test_fma32_rounds_once():
    rng = np.random.default_rng(1)
    a, b, c = (rng.normal(size=20000).astype(F32) for _ in range(3))
    got = spec.fma32(a, b, c)
    # exact in integers: scale to a common exponent with Python's rationals on a sample
    from fractions import Fraction
    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = float(np.nextafter(got[i], F32(-np.inf))), float(np.nextafter(got[i], F32(np.inf)))
        assert abs(exact - Fraction(float(got[i]))) <= min(abs(exact - Fraction(lo)), abs(exact - Fraction(hi)))
    one, odd = np.array([1.0], F32), np.array([1 + 2.0 ** -23], F32)
    lo, hi = np.array([2.0 ** -12 * (1 - 2.0 ** -23)], F32), np.array([2.0 ** -12 * (1 + 2.0 ** -23)], F32)
    # an exact tie goes to the even neighbour: 2^-12 2^-12 + 1 = 1 + 2^-24
    assert spec.fma32(np.array([2.0 ** -12], F32), np.array([2.0 ** -12], F32), one)[0] == F32(1)
    # a hair above the tie goes up: 2^-12 (2^-12 + 2^-35) + 1 = 1 + 2^-24 + 2^-47
    assert spec.fma32(np.array([2.0 ** -12], F32), np.array([2.0 ** -12 + 2.0 ** -35], F32), one)[0] == F32(1 + 2.0 ** -23)
    # a tie the float64 sum alone would decide twice: lo hi + (1 + 2^-23) = 1 + 2^-23 + 2^-24 - 2^-70 lies below the midpoint of 1 + 2^-23
    # and 1 + 2^-22; the float64 sum rounds it ONTO the midpoint, which would then go to the even neighbour 1 + 2^-22
    assert (lo.astype(np.float64) * hi.astype(np.float64) + odd.astype(np.float64)).astype(F32)[0] == F32(1 + 2.0 ** -22)
    assert spec.fma32(lo, hi, odd)[0] == F32(1 + 2.0 ** -23)


def test_a_constant_image_is_constant_exactly():
    rng = np.random.default_rng(2)
    uv = np.concatenate([spec.special_uv(), rng.uniform(-5, 5, (5000, 2)).astype(F32)])
    fin = np.isfinite(uv).all(1)
    for shape in ((4, 4), (7, 5), (16, 32)):
        c = np.array([0.3, 1.7, -0.25], F32)
        im = np.broadcast_to(c, shape + (3,)).copy()
        got = spec.fetch32(im, uv[:, 0], uv[:, 1])
        assert np.array_equal(got[fin].view(np.uint32), np.tile(c, (fin.sum(), 1)).view(np.uint32))
        assert (got[~fin] == 1).all()


def test_a_texel_centre_of_a_power_of_two_image_is_that_texel_exactly():
    for im in (images()[0], images()[1]):
        H, W = im.shape[:2]
        j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        for shift in (0, 3, -2):
            u = ((i.ravel() + 0.5) / W + shift).astype(F32)
            v = ((j.ravel() + 0.5) / H - shift).astype(F32)
            got = spec.fetch32(im, u, v)
            assert np.array_equal(got.view(np.uint32), im.reshape(-1, 3).view(np.uint32))


def test_period_one_in_u_and_v():
    rng = np.random.default_rng(3)
    # multiples of 2^-10 in [0, 1): u + k is exact in fp32 for |k| <= 8, so the two fetches see the same u'
    u = (rng.integers(0, 1024, 4000) / 1024).astype(F32)
    v = (rng.integers(0, 1024, 4000) / 1024).astype(F32)
    for im in images():
        base = spec.fetch32(im, u, v)
        for ku, kv in ((1, 0), (0, 1), (-3, 5), (8, -8)):
            assert np.array_equal(spec.fetch32(im, u + F32(ku), v + F32(kv)).view(np.uint32), base.view(np.uint32))
        got64 = spec.fetch64(im, u.astype(np.float64) + 2, v.astype(np.float64) - 1)
        assert np.abs(got64 - spec.fetch64(im, u, v)).max() <= 1e-12


def test_continuous_across_a_texel_boundary_and_across_the_wrap():
    """Two points h apart differ by at most h x (W + H) x the largest texel step (the bilinear gradient), plus the fetch's own roundings
    (tests/test_gpu_texture.py spells them out: 10 e tmax covers them for |u|, |v| <= 2 and sizes <= 32)."""
    rng = np.random.default_rng(4)
    for im in images():
        H, W = im.shape[:2]
        step, tmax = spec.texel_step(im), float(np.abs(im).max())
        # texel boundaries in x are where x = u' W - 0.5 is an integer: u' = (i + 0.5) / W; the wrap is u = integer
        edges_u = np.concatenate([(np.arange(W) + 0.5) / W, [0.0, 1.0, -1.0, 2.0]])
        edges_v = np.concatenate([(np.arange(H) + 0.5) / H, [0.0, 1.0, -1.0, 2.0]])
        for h in (1e-6, 1e-4):
            for eu in edges_u:
                v = rng.uniform(-1, 2, 16).astype(F32)
                a = spec.fetch32(im, np.full(16, eu - h, F32), v).astype(np.float64)
                b = spec.fetch32(im, np.full(16, eu + h, F32), v).astype(np.float64)
                assert np.abs(a - b).max() <= (2 * h + 4 * E) * W * step + 10 * E * tmax * max(W, H), (im.shape, eu, h)
            for ev in edges_v:
                u = rng.uniform(-1, 2, 16).astype(F32)
                a = spec.fetch32(im, u, np.full(16, ev - h, F32)).astype(np.float64)
                b = spec.fetch32(im, u, np.full(16, ev + h, F32)).astype(np.float64)
                assert np.abs(a - b).max() <= (2 * h + 4 * E) * H * step + 10 * E * tmax * max(W, H), (im.shape, ev, h)


def test_the_fp32_fetch_is_the_float64_statement_within_its_roundings():
    rng = np.random.default_rng(5)
    uv = rng.uniform(-2, 3, (20000, 2)).astype(F32)
    for im in images():
        H, W = im.shape[:2]
        step, tmax = spec.texel_step(im), float(np.abs(im).max())
        err = np.abs(spec.fetch32(im, uv[:, 0], uv[:, 1]).astype(np.float64) - spec.fetch64(im, uv[:, 0], uv[:, 1])).max()
        assert err <= spec.fetch_roundings(im), (im.shape, err, spec.fetch_roundings(im))


def test_two_triangles_sharing_an_edge_and_its_uvs_agree_on_it():
    rng = np.random.default_rng(6)
    k = 4000
    base = spec.random_uv_rows(k)
    p1, p2, p3 = base[:, 0:3], base[:, 3:6], base[:, 6:9]
    uv1, uv2 = base[:, 9:11], base[:, 11:13]
    # the neighbour: the edge p1 p2 the other way round, a third corner of its own with its own uv
    q3 = (p1 + p2 - p3 + rng.normal(size=(k, 3)) * 0.1).astype(F32)
    uvq = rng.uniform(-2, 3, (k, 2)).astype(F32)
    t = rng.uniform(0, 1, (k, 1))
    p = (p1.astype(np.float64) * (1 - t) + p2.astype(np.float64) * t).astype(F32)
    a = np.concatenate([p1, p2, p3, uv1, uv2, base[:, 13:15], p], 1)
    b = np.concatenate([p2, p1, q3, uv2, uv1, uvq, p], 1)
    wa, wb = spec.uv_rows(a), spec.uv_rows(b)
    ok = ~wa["degenerate"] & ~wb["degenerate"]
    assert ok.sum() > 3900
    # in float64 the two agree up to the point's own distance from the edge (p is rounded to fp32: e |p| off it, times the UV gradient)
    ga, gb = spec.uv_rows32(a).astype(np.float64), spec.uv_rows32(b).astype(np.float64)
    assert (np.abs(ga - wa["uv"]) <= wa["D"])[ok].all() and (np.abs(gb - wb["uv"]) <= wb["D"])[ok].all()
    r = base.astype(np.float64)
    d2a, d3a, _ = spec.smooth_spec.duals(r[:, 0:3], r[:, 3:6], r[:, 6:9])
    off = E * np.sqrt((p.astype(np.float64) ** 2).sum(-1)) * np.sqrt(3.0)
    grad_a = (np.sqrt((d2a ** 2).sum(-1))[:, None] * np.abs(r[:, 11:13] - r[:, 9:11]) + np.sqrt((d3a ** 2).sum(-1))[:, None] * np.abs(r[:, 13:15] - r[:, 9:11]))
    rb = b.astype(np.float64)
    d2b, d3b, _ = spec.smooth_spec.duals(rb[:, 0:3], rb[:, 3:6], rb[:, 6:9])
    grad_b = (np.sqrt((d2b ** 2).sum(-1))[:, None] * np.abs(rb[:, 11:13] - rb[:, 9:11]) + np.sqrt((d3b ** 2).sum(-1))[:, None] * np.abs(rb[:, 13:15] - rb[:, 9:11]))
    bound = wa["D"] + wb["D"] + off[:, None] * (grad_a + grad_b)
    assert (np.abs(ga - gb) <= bound)[ok].all(), np.abs(ga - gb)[ok].max()
    assert np.median(bound[ok]) < 1e-5


def test_nan_and_infinite_uvs_give_one():
    im = images()[0]
    nan, inf = F32(np.nan), F32(np.inf)
    u = np.array([nan, inf, -inf, 0.5, 0.5, 0.5, nan, inf], F32)
    v = np.array([0.5, 0.5, 0.5, nan, inf, -inf, nan, -inf], F32)
    assert (spec.fetch32(im, u, v) == 1).all() and (spec.fetch64(im, u, v) == 1).all()


def test_every_index_is_in_range_on_adversarial_inputs():
    """fetch32 asserts the statement's ranges - i0 in [-1, W - 1] before the repeat, every index in [0, n) after it - on every call."""
    uv = spec.special_uv()
    assert len(uv) > 300
    for im in images() + [np.zeros((1, 16384, 3), F32), np.zeros((16384, 1, 3), F32)]:
        got = spec.fetch32(im, uv[:, 0], uv[:, 1])
        assert np.isfinite(got).all()
    # -0 and the largest float below 1, by hand on a 4 x 4 image: u = -0 -> u' = 0 -> x = -0.5 -> i0 = -1 -> W - 1, i1 = 0, fx = 0.5
    im = images()[1][:4, :4].copy()
    below1 = np.nextafter(F32(1), F32(0))
    got = spec.fetch32(im, np.array([-0.0, below1], F32), np.array([0.125, 0.125], F32))
    want0 = spec.fma32(F32(0.5), im[0, 0] - im[0, 3], im[0, 3])
    assert np.array_equal(got[0].view(np.uint32), want0.view(np.uint32))
    # u = 1 - 2^-24: x = fl(4 - 2^-22 - 0.5) = 3.5 - 2^-22 -> 3.4999998 (representable): i0 = 3, i1 = 0 (the wrap), fx just below 0.5
    x = spec.fma32(below1, F32(4), F32(-0.5))
    assert np.floor(x) == 3
    want1 = spec.fma32(x - np.floor(x), im[0, 0] - im[0, 3], im[0, 3])
    assert np.array_equal(got[1].view(np.uint32), want1.view(np.uint32))


def test_a_degenerate_triangle_has_uv1_everywhere():
    rows = np.array([[0, 0, 0, 0, 0, 0, 0, 1, 0, 0.25, 0.75, 0.5, 0.1, 0.9, 0.2, 3, 4, 5],
                     [0, 0, 0, 1, 1, 0, 2, 2, 0, -1.5, 2.5, 0.5, 0.1, 0.9, 0.2, -3, 4, 5]], F32)
    want = spec.uv_rows(rows)
    assert want["degenerate"].all() and np.array_equal(want["uv"], rows[:, 9:11].astype(np.float64))
    assert np.array_equal(spec.uv_rows32(rows).view(np.uint32), rows[:, 9:11].view(np.uint32))
