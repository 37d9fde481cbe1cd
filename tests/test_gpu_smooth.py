"""Smooth shading on the device (include/jade_bvh.h, "The shading normal, stated"; jade_scene_set_vertex_normals): the one function of
(triangle, point, direction) against tests/smooth_spec.py within a derived bound, its closed form on a sphere, the render against the
spec's arm sample for sample (tests/smooth_cases.py), and the denoiser's normal guide.  The seams are in tests/test_gpu_smooth_seams.py.

The bound D of a row, derived before any device run (smooth_spec.normal_rows forms it from the row's float64 quantities).  e = 2^-24.
  d2, d3:  the exact double quotient rounded once: e |d| per vector.   m2 = fl(n2 - n1), m3: e |m| each.   w = fl(p - p1): e |w|.
  b2 = dot(w, d2):  a product and two fmas - 3 e |w||d2| by themselves - on inputs that carry e each: at most 5 e |w||d2|; E_b = 6 e |w||d|.
  s = fma(b3, m3, fma(b2, m2, n1)):  E_b2 |m2| + E_b3 |m3| from the barycentrics, e |b||m| from each m's own rounding, and two fma
      roundings of numbers no larger than |n1| + |b2||m2| + |b3||m3|:  E_s = E_b2 |m2| + E_b3 |m3| + 4 e (|n1| + |b2||m2| + |b3||m3|).
  ns = s / sqrt(ss):  a perturbation E_s of s turns its direction by at most 2 E_s / |s| (the unit vector's change, both its parallel and
      its normal part counted); ss's three roundings, the root's and the quotient's add (1.5 + 0.5 + 1) e on components below 1, and a
      reserve of e:  D = 2 E_s / |s| + 4 e.
On the rows below (edges 0.05 .. 2, no slivers, unit normals) D stays below 2e-4 and is 1.4e-6 in the median.  The side rule's products: a
component error of D is at most sqrt(3) D |r| in dot(ns, r), and the dot itself carries 3 e |r| (+ e reserve); dot(g, r) carries 4 e |g||r|.
A row whose products clear those bounds must report the statement's rule; a row that does not may report RULE_NS or RULE_SIDE, and its
normal is then held to whichever the device reported."""
import ctypes as C

import numpy as np
import pytest

import guide_cases as GC
import jaderaytracerendering_amd as J
import smooth_cases as SC
import smooth_spec as spec
import spec_scenes as SP
from conftest import B
from jaderaytracerendering_amd import _abi, host as H

pytestmark = pytest.mark.gpu
F32 = np.float32
E = 2.0 ** -24


def normal_device(be, rows):
    fn = be.lib.jade_debug_shading_normal
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    rows = np.ascontiguousarray(rows, F32).reshape(-1, 27)
    n = np.full((len(rows), 3), np.nan, F32)
    rule = np.full(len(rows), -1, np.int32)
    be.check(fn(0, len(rows), rows.ctypes.data, n.ctypes.data, rule.ctypes.data))
    return n, rule


def held(rows, got, rule, want):
    """Every row: the rule where it is decided, the normal within the bound (fallback rows: g, bit for bit)."""
    g = rows[:, 18:21]
    decided = want["clear"]
    assert np.array_equal(rule[decided], want["rule"][decided]), np.flatnonzero(decided & (rule != want["rule"]))[:5]
    either = ~decided
    assert np.isin(rule[either], (spec.RULE_NS, spec.RULE_SIDE)).all() and np.isin(want["rule"][either], (spec.RULE_NS, spec.RULE_SIDE)).all()
    fell = rule != spec.RULE_NS
    assert np.array_equal(got[fell].view(np.uint32), g[fell].view(np.uint32)), "a vertex that falls back takes g unchanged"
    ns = rule == spec.RULE_NS
    err = np.abs(got[ns].astype(np.float64) - want["ns"][ns]).max(-1)
    worst = int(np.argmax(err / want["D"][ns]))
    print(f"shading normal: {ns.sum()} interpolated rows, worst error {err[worst]:.3g} against its bound {want['D'][ns][worst]:.3g}; "
          f"median bound {np.median(want['D'][ns]):.3g}, {int(either.sum())} undecided rows")
    assert (err <= want["D"][ns]).all(), (rows[ns][worst], got[ns][worst], want["ns"][ns][worst])
    return ns


def test_device_normal_is_the_statement_within_the_derived_bound(hip_debug):
    rows = np.concatenate([spec.special_rows(), spec.random_rows(24000)])
    assert len(rows) >= 20000
    want = spec.normal_rows(rows)
    got, rule = normal_device(hip_debug, rows)
    ns = held(rows, got, rule, want)
    k = len(spec.special_rows())
    assert list(rule[:k]) == list(want["rule"][:k]), "the special rows take the rule they are written for"
    for r in (spec.RULE_NS, spec.RULE_FLAT, spec.RULE_DEGENERATE, spec.RULE_SUM, spec.RULE_SIDE):
        assert (rule == r).any(), r
    assert ns.sum() > 15000 and (rule == spec.RULE_SIDE).sum() > 2000 and want["clear"].mean() > 0.95
    assert want["D"][ns].max() < 2e-4                  # (a property of the rows, formed in float64 before any device run: 1.2e-4 on these)
    assert np.abs(np.sqrt((got[ns].astype(np.float64) ** 2).sum(-1)) - 1).max() <= 4 * E


def unit_ball():
    """make_geodesic(2) as built, unit and about the origin, with n_i = the vertex itself - signed as the triangle's flat normal points
    (the mesh's winding decides it), so that the side rule keeps it."""
    b = J.SceneBuilder()
    b.add_proc("geodesic", 2, H.material(brdf=(0.7, 0.6, 0.5)))
    b.set_env_constant(0.5, 0.6, 0.8)
    hs = b.build()
    t = hs.tri_f32()
    sign = np.sign((t[:, 10:13] * (t[:, 1:4] + t[:, 4:7] + t[:, 7:10])).sum(-1)).astype(F32)
    assert (np.abs(np.sqrt((t[:, 1:10].reshape(-1, 3).astype(np.float64) ** 2).sum(-1)) - 1) < 1e-6).all()
    hs.vertex_normals = (t[:, 1:10].reshape(-1, 3, 3) * sign[:, None, None]).astype(F32)
    return hs, sign


def test_the_closed_form_on_a_sphere(hip_debug):
    """n_i = v_i on a unit sphere: p = sum b_i v_i, so ns(p) = p / |p| for every point of every triangle, exactly."""
    hs, sign = unit_ball()
    t = hs.tri_f32()
    rng = np.random.default_rng(42)
    per = 64
    b = rng.dirichlet((1, 1, 1), (len(t), per))
    b[:, :3] = np.eye(3)                                            # the corners themselves
    p = (b[..., None] * t[:, None, 1:10].reshape(len(t), 1, 3, 3).astype(np.float64)).sum(2)
    tri = np.repeat(np.arange(len(t)), per)
    p32 = p.reshape(-1, 3).astype(F32)
    r = (p32 * sign[tri][:, None]).astype(F32)                      # on the normals' side
    rows = np.concatenate([t[tri, 1:10], hs.vertex_normals.reshape(-1, 9)[tri], t[tri, 10:13], p32, r], 1)
    want = spec.normal_rows(rows)
    got, rule = normal_device(hip_debug, rows)
    assert (rule == spec.RULE_NS).all() and (want["rule"] == spec.RULE_NS).all()
    held(rows, got, rule, want)
    p64 = p32.astype(np.float64)
    radial = p64 / np.sqrt((p64 * p64).sum(-1))[:, None] * sign[tri][:, None]
    # p32 is p rounded: it lies off its triangle's plane by up to e |p|, which the dual basis drops - the same bound covers it
    err = np.abs(got.astype(np.float64) - radial).max(-1)
    print(f"closed form: {len(rows)} points, worst {err.max():.3g} (bounds {want['D'].min():.3g} .. {want['D'].max():.3g})")
    assert (err <= want["D"] + 2 * E).all()


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_render_is_the_float64_statement_sample_for_sample(hip, name):
    seen, bad, n, skipped, left = SC.run(name, hip)
    assert n + skipped == SC.SIZE * SC.SIZE * len(SC.FRAMES)


def test_the_normal_guide_is_the_shading_normal(hip):
    hs, sign = unit_ball()
    t = hs.tri_f32()
    eye, cam = H.camera_orbit(2.8, 20.0, 10.0)
    G, W = 4, 24
    p = B.make_params(W, W, 1, eye, cam, frame=5)
    with hip.scene(hs) as sc:
        assert sc.vertex_normals_set()
        sc.render(p)
        smooth = sc.guides(G)["normal"]
        # the camera rays of the guide samples (sample s of a pixel is seeded with frame + s) and where they land, by jade_trace_rays
        rays = np.array([[GC.camera_ray(x, y, p, p.frame + s) for s in range(G)] for y in range(W) for x in range(W)])   # [pix, G, (o, d), 3]
        o, d = rays[:, :, 0].reshape(-1, 3), rays[:, :, 1].reshape(-1, 3)
        idx, _, pt, _ = sc.trace_rays(o, d, np.full(len(o), -1, np.int32))
        sc.set_vertex_normals(None)
        assert not sc.vertex_normals_set()
        sc.render(p)
        flat = sc.guides(G)["normal"]
    hit = idx >= 0
    k = np.where(hit, idx, 0)
    rows = np.concatenate([t[k, 1:10], hs.vertex_normals.reshape(-1, 9)[k], t[k, 10:13], pt, (-d).astype(F32)], 1).astype(F32)
    want = spec.normal_rows(rows)
    p64 = pt.astype(np.float64)
    radial = p64 / np.maximum(np.sqrt((p64 * p64).sum(-1)), 1e-30)[:, None]
    facing = -(radial * d).sum(-1)
    # A pixel counts if all its rays hit the ball at more than 0.3 of facing: a camera direction differs by ~3 ulp (2e-7) between the fp32
    # pass and this float64 ray, which moves a hit 3.8 away by 2e-7 x 3.8 / 0.3 = 2.5e-6 on a sphere of radius 1: 3e-6 on the normal,
    # beside the row's own D and the mean's roundings (G e).
    good = (hit & (facing > 0.3) & (want["rule"] == spec.RULE_NS)).reshape(-1, G).all(1)
    assert good.sum() >= 60, good.sum()
    mean_radial = radial.reshape(-1, G, 3).mean(1)
    bound = want["D"].reshape(-1, G).max(1) + 3e-6 + G * E
    got = smooth.reshape(-1, 3).astype(np.float64)
    err = np.abs(got[good] - mean_radial[good]).max(-1)
    print(f"normal guide: {good.sum()} pixels, worst {err.max():.3g} (bound {bound[good].min():.3g} .. {bound[good].max():.3g})")
    assert (err <= bound[good]).all()
    # with the table cleared the guide is the flat normal again: the mean of the triangles' own normals, turned towards the viewer
    g = t[k, 10:13].astype(np.float64)
    g = np.where(((g * d).sum(-1) > 0)[:, None], -g, g)
    mean_flat = g.reshape(-1, G, 3).mean(1)
    errf = np.abs(flat.reshape(-1, 3).astype(np.float64)[good] - mean_flat[good]).max(-1)
    assert (errf <= (G + 1) * E).mean() >= 0.95, errf.max()    # (a ray within an ulp of an edge may land on the neighbour in one of the two passes)
    assert np.abs(mean_flat[good] - mean_radial[good]).max() > 0.02, "and the two guides differ on an 80-triangle ball"
