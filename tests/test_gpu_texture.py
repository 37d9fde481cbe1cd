"""Albedo textures on the device (include/jade_bvh.h, "The surface colour, stated"; jade_scene_set_textures): the fetch against
tests/texture_spec.py's emulated fp32 bit for bit, the lookup and the surface colour within bounds derived before any device run, the
render against the spec's arm sample for sample (tests/texture_cases.py), a closed form on a ramp-textured floor, and the denoiser's
albedo guide.  The seams are in tests/test_gpu_texture_seams.py.

The bounds, e = 2^-24.
  uv(triangle, p), per component (texture_spec.uv_rows forms D from the row's float64 quantities, as tests/test_gpu_smooth.py does for the
  normal): d2, d3 the exact double quotient rounded once, e |d|; w = fl(p - p1), e |w|; b2 = dot(w, d2), a product and two fmas on inputs
  that carry e each: E_b = 6 e |w||d|.  du2 = fl(uv2 - uv1): e |du2|.  u = fma(b3, du3.x, fma(b2, du2.x, u1)): E_b2 |du2.x| + E_b3 |du3.x|
  from the barycentrics, e |b||du| from each du's own rounding and two fma roundings of numbers no larger than |u1| + |b2||du2.x| +
  |b3||du3.x|:   D_u = E_b2 |du2.x| + E_b3 |du3.x| + 4 e (|u1| + |b2||du2.x| + |b3||du3.x|).
  The surface colour: the fetch is continuous and piecewise linear in (u, v) with slope at most W step per unit of u and H step per unit
  of v (step: the largest difference of neighbouring texels, the wrap included), so the device's fp32 (u, v) moves it by at most
  (D_u W + D_v H) step <= (D_u + D_v) max(W, H) step; the fetch's own roundings are texture_spec.fetch_roundings (derived there)."""
import ctypes as C
import math

import numpy as np
import pytest

import jaderaytracerendering_amd as J
import spec_scenes as SP
import texture_cases as TC
import texture_spec as spec
from conftest import B
from jaderaytracerendering_amd import _abi, host as H
from render_helpers import same_bits
from texture_cases import FLOOR_S, FLOOR_Y, WALL_S, WALL_Y, corner_ray, mirror_and_wall

pytestmark = pytest.mark.gpu
F32 = np.float32
E = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ the function --
def _call(be, name, sc, index, floats, per_row, out_cols):
    fn = getattr(be.lib, name)
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    index = np.ascontiguousarray(index, np.int32)
    floats = np.ascontiguousarray(floats, F32).reshape(len(index), per_row)
    out = np.full((len(index), out_cols), np.nan, F32)
    be.check(fn(sc._h, len(index), index.ctypes.data, floats.ctypes.data, out.ctypes.data))
    return out


def fetch_device(be, sc, image, uv):
    return _call(be, "jade_debug_texture_fetch", sc, image, uv, 2, 3)


def uv_device(be, sc, tri, p):
    return _call(be, "jade_debug_surface_uv", sc, tri, p, 3, 2)


def colour_device(be, sc, tri, p):
    return _call(be, "jade_debug_surface_colour", sc, tri, p, 3, 3)


def fetch_images():
    rng = np.random.default_rng(7)
    return [rng.uniform(-0.5, 2.0, s).astype(F32) for s in ((4, 8, 3), (16, 16, 3), (5, 7, 3), (1, 1, 3), (32, 3, 3), (4, 4, 3))]


def test_device_fetch_is_the_emulated_fp32_statement_bit_for_bit(hip_debug):
    images = fetch_images()
    images[5][:] = np.array([0.3, 1.7, -0.25], F32)                     # a constant image
    hs = SP.build("open_floor")
    TC.textured(hs, images, image_of=np.arange(hs.n_triangles) % len(images))
    rng = np.random.default_rng(8)
    special = spec.special_uv()
    # the special rows on every image, texel centres and boundaries of every image with a few wraps, and random rows in [-3, 4]
    image, uv = [], []
    for k, im in enumerate(images):
        Hh, W = im.shape[:2]
        j, i = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
        centres = np.stack([(i.ravel() + 0.5) / W, (j.ravel() + 0.5) / Hh], 1)
        edges = np.stack([i.ravel() / W, j.ravel() / Hh], 1)
        block = np.concatenate([special, centres, centres + (3, -2), edges, edges - (1, 0), rng.uniform(-3, 4, (3600, 2))]).astype(F32)
        uv.append(block)
        image.append(np.full(len(block), k, np.int32))
    image, uv = np.concatenate(image), np.concatenate(uv)
    assert len(uv) >= 20000
    want = np.zeros((len(uv), 3), F32)
    for k, im in enumerate(images):
        m = image == k
        want[m] = spec.fetch32(im, uv[m, 0], uv[m, 1])
    with hip_debug.scene(hs) as sc:
        got = fetch_device(hip_debug, sc, image, uv)
    same = (got.view(np.uint32) == want.view(np.uint32)).all(1)
    print(f"texture fetch: {len(uv)} rows on {len(images)} images, {int((~same).sum())} differ")
    assert same.all(), (image[~same][:5], uv[~same][:5], got[~same][:5], want[~same][:5])
    bad = ~np.isfinite(uv).all(1)
    assert bad.sum() >= 15 * len(images) and (got[bad] == 1).all()
    const = image == 5
    assert (got[const & ~bad] == images[5][0, 0]).all(), "a constant image is its constant exactly"


def soup(k=24000, seed=953):
    """k random triangles (smooth_spec.random_rows': edges 0.05 .. 2, no slivers) as one diffuse mesh: the scene whose table the lookup is asked
    on (nothing renders it).  Returns the host scene with UVs in [-2, 3], two images of different sizes dealt over the triangles and a
    quarter of them left without, and a handful of triangles made degenerate in the record (two corners equal; three in a line)."""
    rows = spec.smooth_spec.random_rows(k, seed)
    b = J.SceneBuilder()
    try:
        b.add_mesh(rows[:, 0:9].reshape(-1, 3), np.arange(3 * k, dtype=np.int32).reshape(-1, 3), H.material(brdf=(0.7, 0.6, 0.5)))
        b.set_env_constant(0.5, 0.6, 0.8)
        hs = b.build()
    finally:
        b.close()
    t = hs.tri_f32()
    t[0:4, 4:7] = t[0:4, 1:4]                                       # p2 = p1
    for i in range(4, 8):                                           # three in a line, exactly
        t[i, 1:10] = [i, 0, 0, i + 1, 1, 0, i + 2, 2, 0]
    t[8:12, 7:10] = t[8:12, 4:7] = t[8:12, 1:4]                    # a point
    rng = np.random.default_rng(seed + 1)
    uv = rng.uniform(-2, 3, (hs.n_triangles, 3, 2)).astype(F32)
    image_of = rng.integers(-1, 2, hs.n_triangles).astype(np.int32)
    image_of[rng.random(hs.n_triangles) < 0.25] = -1
    image_of[:12] = 0
    images = [rng.uniform(0.0, 1.5, (16, 16, 3)).astype(F32), rng.uniform(0.0, 1.5, (8, 32, 3)).astype(F32)]
    return TC.textured(hs, images, image_of, uv)


@pytest.fixture(scope="module")
def soup_rows():
    """(host scene, tri [n], rows [n, 18], want = spec.uv_rows(rows)): three points per triangle - inside, up to 5 % outside - formed
    before any device run."""
    hs = soup()
    n = hs.n_triangles
    rng = np.random.default_rng(954)
    tri = np.repeat(np.arange(n, dtype=np.int32), 3)
    v = hs.vertices().astype(np.float64)[tri]
    b = rng.dirichlet((1, 1, 1), len(tri)) * 1.1 - 0.05
    b[:, 0] = 1 - b[:, 1] - b[:, 2]
    p = (b[:, :, None] * v).sum(1).astype(F32)
    rows = np.concatenate([hs.vertices()[tri].reshape(-1, 9), hs.textures[1][tri].reshape(-1, 6), p], 1).astype(F32)
    return hs, tri, rows, spec.uv_rows(rows)


def test_device_uv_is_the_statement_within_the_derived_bound(hip_debug, soup_rows):
    hs, tri, rows, want = soup_rows
    assert len(rows) >= 20000 and want["degenerate"].sum() >= 24
    assert want["D"][~want["degenerate"]].max() < 2e-3       # (a property of the rows: triangles down to 0.05 with |uv| up to 3 and |du| up to 5)
    with hip_debug.scene(hs) as sc:
        got = uv_device(hip_debug, sc, tri, rows[:, 15:18])
    deg = want["degenerate"]
    assert np.array_equal(got[deg].view(np.uint32), rows[deg, 9:11].view(np.uint32)), "every point of a degenerate triangle has uv1"
    err = np.abs(got.astype(np.float64) - want["uv"])[~deg]
    D = want["D"][~deg]
    worst = np.unravel_index(np.argmax(err / D), err.shape)
    print(f"surface uv: {len(err)} rows, worst error {err[worst]:.3g} against its bound {D[worst]:.3g} (ratio {err[worst] / D[worst]:.3g}); "
          f"median bound {np.median(D):.3g}, largest {D.max():.3g}")
    assert (err <= D).all(), (rows[~deg][worst[0]], got[~deg][worst[0]], want["uv"][~deg][worst[0]])
    # ... and the statement's own fp32 operations give the device's bits (d2, d3 are rounded once from the same doubles)
    same = (spec.uv_rows32(rows).view(np.uint32) == got.view(np.uint32)).all(1)
    assert same.mean() > 0.999, same.mean()


def test_device_surface_colour_is_within_the_uv_bound_times_the_texel_step(hip_debug, soup_rows):
    hs, tri, rows, want = soup_rows
    images, _, image_of = hs.textures
    with hip_debug.scene(hs) as sc:
        got = colour_device(hip_debug, sc, tri, rows[:, 15:18])
    im = image_of[tri]
    none = im < 0
    assert none.sum() > 5000 and (got[none] == 1).all(), "a triangle without an image has c = (1, 1, 1)"
    n_checked = 0
    for k, image in enumerate(images):
        m = im == k
        Hh, W = image.shape[:2]
        ref = spec.fetch64(image, want["uv"][m, 0], want["uv"][m, 1])
        bound = (want["D"][m, 0] * W + want["D"][m, 1] * Hh) * spec.texel_step(image) + spec.fetch_roundings(image)
        err = np.abs(got[m].astype(np.float64) - ref).max(1)
        worst = int(np.argmax(err / bound))
        print(f"surface colour, image {k} ({W} x {Hh}): {m.sum()} rows, worst error {err[worst]:.3g} against its bound {bound[worst]:.3g}")
        assert (err <= bound).all(), (rows[m][worst], got[m][worst], ref[worst])     # bilinear filtering is continuous: no row is left out
        n_checked += int(m.sum())
    assert n_checked + none.sum() == len(rows) and n_checked >= 20000


# -------------------------------------------------------------------------------------------------------------------- the render --
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_render_is_the_float64_statement_sample_for_sample(hip, name):
    seen, bad, n, skipped = TC.run(name, hip)
    assert n + skipped == TC.SIZE * TC.SIZE * len(TC.FRAMES)


RAMP_W = 16
U_CENTRE, DU_DX = 1.0, 1.0 / 9.0


def u_bound(hs, which, pts):
    """The largest D_u (texture_spec.uv_rows) of the points pts on the triangles `which` of hs: |w|, |b2| and |b3| are convex in the point, so
    the corners of a convex footprint bound every point inside it."""
    tri = np.flatnonzero(which)
    rows = np.concatenate([np.repeat(hs.vertices()[tri].reshape(-1, 9), len(pts), 0), np.repeat(hs.textures[1][tri].reshape(-1, 6), len(pts), 0),
                           np.tile(pts, (len(tri), 1))], 1)
    return float(spec.uv_rows(rows.astype(F32))["D"][:, 0].max())


def ramp_image():
    """16 x 4, texel (i, j) = base + slope i per channel (all multiples of 1/64): the filter of a ramp is affine in u away from the wrap -
    for u in [0.5 / 16, 1 - 0.5 / 16] - and does not depend on v."""
    i = np.arange(RAMP_W, dtype=np.float64)
    row = np.stack([0.25 + i / 32, 1.0 - i / 64, 0.5 + i / 16], 1)
    return np.broadcast_to(row, (4, RAMP_W, 3)).astype(F32).copy()


def ramp_floor():
    """A diffuse floor with brdf 1 under a constant sky, no emitter; u = 0.5 + (x - 1) / 9, v = 0.5 + (z - 1) / 9: the part of the floor the
    camera below sees has u in [0.1, 0.9] (the test asserts it pixel by pixel), most of the ramp."""
    b = J.SceneBuilder()
    try:
        b.add_mesh(SP.quad(FLOOR_Y, FLOOR_S), SP.QUAD_I, H.material(brdf=(1, 1, 1)))
        b.set_env_constant(0.5, 0.6, 0.8)
        hs = b.build()
    finally:
        b.close()
    v = hs.vertices().astype(np.float64)
    uv = (0.5 + (v[:, :, [0, 2]] - U_CENTRE) * DU_DX).astype(F32)
    return TC.textured(hs, [ramp_image()], uv=uv)


def test_the_closed_form_on_a_ramp_textured_floor(hip):
    """brdf 1, a constant sky S, no emitter, JADE_BOUNCE_COSINE: a sample's vertex on the floor sends its environment ray into the open sky
    and its indirect ray too, so the sample is S c(p) K with K the chain's constant (below); the pixel is the mean of its samples, and c is
    affine over the floor, so the pixel lies between the least and the largest corner value of its footprint - a convex quadrilateral,
    the image of the pixel's square under the camera's projective map.  Widened by, relative to the value:
      brdf_eff = fl(1 c) = c exactly; f = brdf_eff fl(1 / pi): 2 e (the constant's rounding and the product's); the sky times f: e; the
      cosine weight sqrt(n.n) / 2 of the floor's unit normal (n.n within 4 e + 1.5 e of 1, the root halves it and rounds, the product
      rounds): 5 e; times 2, exact; times fl(pi): 2 e; the path's fold thr l (thr = 1) + 0: exact; the sum of spp samples: spp e; the mean: e.
      In all (11 + spp) e, taken as (16 + spp) e.
    and, absolute: the colour's own error at the device's point - (D_u W) step + the fetch's roundings (the module docstring) - and the
    point's: the fp32 camera direction is off by 4 e, which moves a hit t away by 4 e t / cos, and the hit point rounds its coordinates,
    8 e R with R the largest coordinate in play; times |du / dx| W step."""
    hs = ramp_floor()
    image = hs.textures[0][0]
    eye, cam = H.camera_orbit(3.0, 65.0, 25.0)
    W, spp = 16, 16
    p = B.make_params(W, W, spp, eye, cam, frame=2)
    sky = np.array([0.5, 0.6, 0.8], F32).astype(np.float64)
    K = float(F32(1.0 / math.pi)) * 0.5 * 2.0 * float(F32(math.pi))
    slope = (image[0, 1].astype(np.float64) - image[0, 0])             # per texel
    base = image[0, 0].astype(np.float64)
    du_dx = DU_DX
    lo, hi = np.zeros((W, W, 3)), np.zeros((W, W, 3))
    for y in range(W):
        for x in range(W):
            pts, reach = [], 0.0
            for rx in (0, 1):
                for ry in (0, 1):
                    o, d = corner_ray(p, x, y, rx, ry)
                    assert d[1] < -0.2, "every corner ray goes down to the floor"
                    t = (FLOOR_Y - o[1]) / d[1]
                    q = o + t * d
                    assert np.abs(q[[0, 2]]).max() < FLOOR_S - 0.1, "... and lands on it"
                    pts.append(q)
                    reach = max(reach, 4 * E * t / -d[1] + 8 * E * max(np.abs(o).max(), np.abs(q).max()))
            pts = np.array(pts)
            u = 0.5 + (pts[:, 0] - U_CENTRE) * du_dx
            assert u.min() > 0.5 / RAMP_W and u.max() < 1 - 0.5 / RAMP_W
            c = base[None] + slope[None] * (u[:, None] * RAMP_W - 0.5)         # the filter of the ramp, in float64
            D = u_bound(hs, np.ones(hs.n_triangles, bool), pts)
            widen = ((D + reach * du_dx) * RAMP_W) * np.abs(slope) + spec.fetch_roundings(image)
            rel = (16 + spp) * E
            lo[y, x] = sky * K * (c.min(0) - widen) * (1 - rel)
            hi[y, x] = sky * K * (c.max(0) + widen) * (1 + rel)
    with hip.scene(hs) as sc:
        sc.set_bounce_sampling(_abi.BOUNCE_COSINE)
        rgb, _, st = sc.render(p, want_bgr8=False)
        assert st.samples == W * W * spp and st.rays_inline == 0
    got = rgb.astype(np.float64)
    inside = (got >= lo) & (got <= hi)
    width = (hi - lo) / np.maximum(hi, 1e-30)
    print(f"closed form: {W * W} pixels, {int((~inside).sum())} channel values outside; bracket width {width.min():.3g} .. {width.max():.3g} of the value")
    assert inside.all(), (np.argwhere(~inside)[:4], got[~inside][:4], lo[~inside][:4], hi[~inside][:4])
    assert np.median(width) < 0.2 and got[..., 0].max() > 1.5 * got[..., 0].min(), "the ramp shows, and the bracket is narrow against it"


# --------------------------------------------------------------------------------------------------------------------- the guide --
FLOOR_TINT = np.array([0.5, 0.75, 0.875], F32)


def test_the_albedo_guide_is_the_product_of_the_chains_effective_brdfs(hip):
    """The guide pass follows the mirror floor to the wall: albedo = brdf_eff(floor) brdf_eff(wall), the mean of G samples.  The floor's
    image is constant, the wall's a ramp, so the product is affine over the wall; the mirror image of a pinhole camera is a pinhole camera,
    so a pixel's footprint on the wall is the quadrilateral of its four reflected corner rays and the guide lies between the least and the
    largest corner value - widened as in the closed form: two products and the mean's G + 1 roundings relative ((G + 8) e taken), the
    colour's error and the point's absolute."""
    floor_image = np.broadcast_to(FLOOR_TINT, (4, 4, 3)).copy()
    image = ramp_image()
    hs, is_wall = mirror_and_wall(image, floor_image)
    eye, cam = H.camera_orbit(2.0, 50.0, 25.0)
    W, G = 12, 4
    p = B.make_params(W, W, 1, eye, cam, frame=5)
    t = hs.tri_f32()
    brdf_floor = t[~is_wall][0, 16:19].astype(np.float64) * FLOOR_TINT.astype(np.float64)
    brdf_wall = t[is_wall][0, 16:19].astype(np.float64)
    slope, base = image[0, 1].astype(np.float64) - image[0, 0], image[0, 0].astype(np.float64)
    du_dx = 1.0 / (2.4 * WALL_S)
    lo, hi = np.zeros((W, W, 3)), np.zeros((W, W, 3))
    for y in range(W):
        for x in range(W):
            us, pts, reach = [], [], 0.0
            for rx in (0, 1):
                for ry in (0, 1):
                    o, d = corner_ray(p, x, y, rx, ry)
                    assert d[1] < -0.2, "every corner ray goes down to the floor"
                    t1 = (FLOOR_Y - o[1]) / d[1]
                    q = o + t1 * d
                    r = d * np.array([1.0, -1.0, 1.0])                           # reflected about the floor's normal (0, 1, 0): up to the wall
                    assert np.abs(q[[0, 2]]).max() < FLOOR_S - 0.1
                    t2 = (WALL_Y - q[1]) / r[1]
                    w = q + t2 * r
                    assert np.abs(w[[0, 2]]).max() < WALL_S - 0.1
                    us.append(0.5 + w[0] * du_dx)
                    pts.append(w)
                    reach = max(reach, 4 * E * (t1 + t2) / r[1] + 16 * E * max(np.abs(o).max(), np.abs(q).max(), np.abs(w).max()))
            us = np.array(us)
            assert us.min() > 0.5 / RAMP_W and us.max() < 1 - 0.5 / RAMP_W
            c = base[None] + slope[None] * (us[:, None] * RAMP_W - 0.5)
            D = u_bound(hs, is_wall, np.array(pts))
            widen = ((D + reach * du_dx) * RAMP_W) * np.abs(slope) + spec.fetch_roundings(image)
            rel = (G + 8) * E
            lo[y, x] = brdf_floor * brdf_wall * (c.min(0) - widen) * (1 - rel)
            hi[y, x] = brdf_floor * brdf_wall * (c.max(0) + widen) * (1 + rel)
    with hip.scene(hs) as sc:
        sc.render(p)
        got = sc.guides(G)["albedo"].reshape(W, W, 3).astype(np.float64)
        # a constant image on the wall as well: the guides of the scene with both constants baked in, bit for bit
        wall_tint = np.array([1.25, 0.5, 0.75], F32)
        sc.set_textures([np.broadcast_to(wall_tint, (8, 8, 3)).copy(), floor_image], hs.textures[1], hs.textures[2])
        sc.render(p)
        const = sc.guides(G)
    c = np.where(is_wall[:, None], wall_tint, FLOOR_TINT)
    with hip.scene(TC.baked(hs, c)) as sb:
        assert not sb.textures
        sb.render(p)
        flat = sb.guides(G)
    inside = (got >= lo) & (got <= hi)
    print(f"albedo guide: {W * W} pixels, {int((~inside).sum())} channel values outside")
    assert inside.all(), (np.argwhere(~inside)[:4], got[~inside][:4], lo[~inside][:4], hi[~inside][:4])
    for k in flat:
        assert same_bits(const[k], flat[k]), k
