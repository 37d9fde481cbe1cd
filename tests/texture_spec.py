"""Albedo textures (include/jade_bvh.h, "The surface colour, stated"; jade_scene_set_textures), written from the header's text and NOT
from csrc/jade_texture.h or the kernels.

fetch32(image, u, v): the texel colour op by op in emulated fp32 - what the device must return bit for bit.  numpy's float32 +, -, * and
floor are IEEE operations; fma32 is the float64 product of two floats (exact: 24 x 24 bits) plus a float, rounded ONCE to fp32 - as
bounce_spec and test_fpmath form it, made exact here: the float64 sum's own rounding error is recovered (TwoSum) and the sum is rounded
to odd before it is rounded to fp32, so no tie is decided twice.
fetch64(image, u, v): the same statement in float64 (bilinear, repeat) - continuous in (u, v), which is what the bounds lean on.
uv_rows(rows): uv(triangle, p) in float64 on rows of 18 fp32 numbers - p1 p2 p3 uv1 uv2 uv3 p - with the row's error bound D
(tests/test_gpu_texture.py derives it).
colour(images, uv, image_of, tri rows, p): the surface colour in float64.
sample(...): smooth_spec.sample with the colour read at (triangle, point) wherever the arm reads brdf or refract_albedo."""
import math

import numpy as np

import jade_spec
import smooth_spec
from jade_spec import PI, SSS

F32 = np.float32
E = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- emulated fp32 --
def fma32(a, b, c):
    """fma(a, b, c) on float32 arrays, correctly rounded."""
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                   # exact
        s = p + c
        bb = s - p                                  # TwoSum: s + err == p + c exactly (where everything is finite)
        err = (p - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        even = (np.atleast_1d(s).view(np.uint64) & np.uint64(1)) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s_odd = np.where(inexact & even.reshape(np.shape(s)), np.nextafter(s, toward), s)
        return s_odd.astype(F32)


def dot32(a, b):
    """The header's dot on rows [k, 3] of float32."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(all="ignore"):
        return fma32(a[:, 2], b[:, 2], fma32(a[:, 1], b[:, 1], a[:, 0] * b[:, 0]))


def _axis32(u, n):
    """One axis of the fetch: (i0, i1, f) for float32 u (finite) and a size n."""
    with np.errstate(all="ignore"):
        up = (u - np.floor(u)).astype(F32)
        x = fma32(up, np.full(u.shape, n, F32), np.full(u.shape, -0.5, F32))
        xf = np.floor(x)
        f = (x - xf).astype(F32)
    i0 = xf.astype(np.int64)
    assert ((i0 >= -1) & (i0 <= n - 1)).all(), "the statement's range of i0"
    i1 = i0 + 1
    i0 = np.where(i0 < 0, n - 1, i0)
    i1 = np.where(i1 == n, 0, i1)
    assert ((i0 >= 0) & (i0 < n) & (i1 >= 0) & (i1 < n)).all(), "every index is in range"
    return i0, i1, f


def fetch32(image, u, v):
    """image float32 [H, W, 3] (row 0 at v = 0), u and v float32 [k] -> float32 [k, 3]."""
    image = np.asarray(image, F32)
    u, v = np.asarray(u, F32).reshape(-1), np.asarray(v, F32).reshape(-1)
    H, W = image.shape[:2]
    ok = np.isfinite(u) & np.isfinite(v)
    uu, vv = np.where(ok, u, F32(0)), np.where(ok, v, F32(0))
    i0, i1, fx = _axis32(uu, W)
    j0, j1, fy = _axis32(vv, H)
    fx, fy = fx[:, None], fy[:, None]
    t00, t10, t01, t11 = image[j0, i0], image[j0, i1], image[j1, i0], image[j1, i1]
    top = fma32(fx, t10 - t00, t00)
    bottom = fma32(fx, t11 - t01, t01)
    c = fma32(fy, bottom - top, top)
    return np.where(ok[:, None], c, F32(1)).astype(F32)


# -------------------------------------------------------------------------------------------------------------------- float64 --
def _axis64(u, n):
    up = u - np.floor(u)
    x = up * n - 0.5
    xf = np.floor(x)
    i0 = xf.astype(np.int64)
    return np.mod(i0, n), np.mod(i0 + 1, n), x - xf


def fetch64(image, u, v):
    """The statement in float64: image [H, W, 3], u and v float64 [k] -> float64 [k, 3]; (1, 1, 1) where u or v is not finite."""
    image = np.asarray(image, np.float64)
    u, v = np.asarray(u, np.float64).reshape(-1), np.asarray(v, np.float64).reshape(-1)
    H, W = image.shape[:2]
    ok = np.isfinite(u) & np.isfinite(v)
    i0, i1, fx = _axis64(np.where(ok, u, 0.0), W)
    j0, j1, fy = _axis64(np.where(ok, v, 0.0), H)
    fx, fy = fx[:, None], fy[:, None]
    top = image[j0, i0] + fx * (image[j0, i1] - image[j0, i0])
    bottom = image[j1, i0] + fx * (image[j1, i1] - image[j1, i0])
    return np.where(ok[:, None], top + fy * (bottom - top), 1.0)


def texel_step(image):
    """The largest difference between two texels that are neighbours in a row or in a column, the wrap included, over the channels."""
    im = np.asarray(image, np.float64)
    return float(max(np.abs(im - np.roll(im, 1, 0)).max(), np.abs(im - np.roll(im, 1, 1)).max()))


def fetch_roundings(image):
    """The bound on |fetch32 - fetch64| at one fp32 (u, v), e = 2^-24, step = texel_step, tmax = the largest |texel|:
      u' = fl(u - floor(u)) lies in [0, 1]: e.   x = fma(u', W, -0.5): the error of u' times W and one rounding of a number below W: 2 e W
      texels in all; floor and fx = x - xf are exact.  A shift of x by d texels moves the filtered colour by at most d step (the filter
      is continuous and piecewise linear with slope <= step per texel, across texel boundaries and the wrap too): (2 W + 2 H) e step.
      Then per channel: each difference of neighbours e step, top and bottom one fma rounding e tmax each, their difference 2 e tmax at
      most, the last fma e tmax:  2 e step + 5 e tmax; one e tmax in reserve."""
    H, W = np.asarray(image).shape[:2]
    return (2 * W + 2 * H + 2) * E * texel_step(image) + 6 * E * float(np.abs(np.asarray(image, np.float64)).max())


def _len(v):
    return np.sqrt((v * v).sum(-1))


def uv_rows(rows):
    """rows fp32 [k, 18]: p1 p2 p3 (9) uv1 uv2 uv3 (6) p (3) -> dict(uv [k, 2] float64, D [k, 2] the bound on (u, v), degenerate [k])."""
    rows = np.asarray(rows, F32).reshape(-1, 18)
    r = rows.astype(np.float64)
    p1, p2, p3 = r[:, 0:3], r[:, 3:6], r[:, 6:9]
    uv1, uv2, uv3, p = r[:, 9:11], r[:, 11:13], r[:, 13:15], r[:, 15:18]
    d2, d3, NN = smooth_spec.duals(p1, p2, p3)
    with np.errstate(all="ignore"):
        degenerate = ~((NN > 0) & (NN < np.inf))
        d2 = np.where(degenerate[:, None], 0.0, d2)
        d3 = np.where(degenerate[:, None], 0.0, d3)
        w = p - p1
        b2, b3 = (w * d2).sum(-1), (w * d3).sum(-1)
        du2, du3 = uv2 - uv1, uv3 - uv1
        uv = uv1 + b2[:, None] * du2 + b3[:, None] * du3
        lw = _len(w)
        eb2, eb3 = 6 * E * lw * _len(d2), 6 * E * lw * _len(d3)
        D = eb2[:, None] * np.abs(du2) + eb3[:, None] * np.abs(du3) + 4 * E * (np.abs(uv1) + np.abs(b2)[:, None] * np.abs(du2) + np.abs(b3)[:, None] * np.abs(du3))
    return dict(uv=uv, D=D, degenerate=degenerate)


def uv_rows32(rows):
    """The same rows through the statement's fp32 operations: the record (d2, d3 formed in double and rounded once, du2 and du3 one
    subtraction) and uv(triangle, p) -> float32 [k, 2]."""
    rows = np.asarray(rows, F32).reshape(-1, 18)
    r = rows.astype(np.float64)
    d2, d3, NN = smooth_spec.duals(r[:, 0:3], r[:, 3:6], r[:, 6:9])
    with np.errstate(all="ignore"):
        degenerate = ~((NN > 0) & (NN < np.inf))
        d2 = np.where(degenerate[:, None], 0.0, d2).astype(F32)
        d3 = np.where(degenerate[:, None], 0.0, d3).astype(F32)
        w = rows[:, 15:18] - rows[:, 0:3]
        du2, du3 = rows[:, 11:13] - rows[:, 9:11], rows[:, 13:15] - rows[:, 9:11]
    b2, b3 = dot32(w, d2), dot32(w, d3)
    return np.stack([fma32(b3, du3[:, i], fma32(b2, du2[:, i], rows[:, 9 + i])) for i in (0, 1)], 1)


def random_uv_rows(k, seed=951):
    """smooth_spec.random_rows' triangles and points (edges 0.05 .. 2, no slivers, points inside and up to 5 % outside) with corner UVs in
    [-2, 3], so that wrap seams cross many triangles."""
    base = smooth_spec.random_rows(k, seed)
    rng = np.random.default_rng(seed + 1)
    uv = rng.uniform(-2, 3, (k, 6)).astype(F32)
    return np.concatenate([base[:, 0:9], uv, base[:, 21:24]], 1).astype(F32)


def special_uv():
    """(u, v) pairs whose handling does not depend on a rounding: -0, the largest float below 1, +-2^30, denormals of both signs, texel
    centres and texel boundaries of an 8 x 4 image, the wrap, NaN and the infinities."""
    tiny = float(np.finfo(F32).smallest_subnormal)
    below1 = float(np.nextafter(F32(1), F32(0)))
    us = [-0.0, 0.0, below1, -below1, 1.0, -1.0, 2.0 ** 30, -2.0 ** 30, 2.0 ** 30 + 128, tiny, -tiny, 1e-39, -1e-39, float(np.finfo(F32).tiny), -float(np.finfo(F32).tiny),
          float(np.finfo(F32).max), -float(np.finfo(F32).max), 0.5, 0.0625, 0.9375, 0.125, 0.25, 0.875, 0.375, -0.0625, 1.0625, 3.4375, -7.8125, 1e-8, -1e-8, 8388608.5,
          16777216.0, -16777215.0, 0.99999, -0.99999, 5e-8, 0.062499996, 0.06250001]
    bad = [float("nan"), float("inf"), float("-inf")]
    rows = [(a, b) for a in us for b in (0.3, -0.0, below1, 0.125, 0.375, -tiny, 2.0 ** 30)] + [(b, a) for a in us for b in (0.7, 0.0625)]
    rows += [(a, 0.5) for a in bad] + [(0.5, a) for a in bad] + [(a, b) for a in bad for b in bad]
    return np.array(rows, F32)


# ------------------------------------------------------------------------------------------------------------------ the render --
class Scene(smooth_spec.Scene):
    """smooth_spec.Scene plus the host scene's textures: hs.textures = (images, uv [n, 3, 2], image_of [n]) or None."""

    def __init__(self, hs, env_sampling=0, light_sampling=0, cosine=False):
        super().__init__(hs, env_sampling, light_sampling, cosine)
        tex = getattr(hs, "textures", None)
        n = len(self.tri32)
        if tex is None:
            self.images, self.uv32, self.image_of = [], np.zeros((n, 6), F32), np.full(n, -1, np.int64)
        else:
            self.images = [np.asarray(im, F32).astype(np.float64) for im in tex[0]]
            self.uv32 = np.ascontiguousarray(tex[1], F32).reshape(n, 6)
            self.image_of = np.asarray(tex[2], np.int64).reshape(n)


def colour(S, k, p):
    """c(triangle k, p) of the header in float64."""
    im = int(S.image_of[k])
    if im < 0:
        return np.ones(3)
    row = np.concatenate([S.tri32[k, :9], S.uv32[k], np.asarray(p, np.float64)])       # (p stays float64 below)
    r = row.astype(np.float64)
    d2, d3, NN = smooth_spec.duals(r[None, 0:3], r[None, 3:6], r[None, 6:9])
    if not (NN[0] > 0 and NN[0] < np.inf):
        uv = r[9:11]
    else:
        w = np.asarray(p, np.float64) - r[0:3]
        b2, b3 = float(w @ d2[0]), float(w @ d3[0])
        uv = r[9:11] + b2 * (r[11:13] - r[9:11]) + b3 * (r[13:15] - r[9:11])
    return fetch64(S.images[im], uv[0:1], uv[1:2])[0]


def path_tracing(S, rng, obj, src, out, trace):
    """smooth_spec.path_tracing with the material at the vertex: brdf_eff = brdf * c, albedo_eff = refract_albedo * c, c = colour(obj, src)."""
    sm = smooth_spec
    stack = []
    L = np.zeros(3)
    while len(stack) < 128:
        if jade_spec.emissive(S, obj, 1.4e-5):
            L = S.emis[obj].copy()
            break
        L = np.zeros(3)
        g = S.norm[obj]
        c = colour(S, obj, src)
        if int(S.image_of[obj]) >= 0:
            trace.append("textured")
        fr = S.brdf[obj] * c * float(F32(1.0 / PI))
        k = 2 if S.refract[obj] != 0 else 1
        u = next(rng)
        if u < 0.5 and S.refract[obj] != 0:
            if S.refract[obj] == 1:
                if next(rng) < SSS:
                    trace.append("sss")
                    fa = S.albedo[obj] * c * float(F32(1.0 / PI))
                    L, nxt = sm.diffuse_like(S, rng, obj, src, out, sm.normal(S, obj, src, out, trace, g), g, fa, fr, k / SSS, trace)
                else:
                    trace.append("bssrdf")
                    L, nxt = sm.bssrdf(S, rng, obj, src, out, sm.normal(S, obj, src, out, trace, g), k, trace)
            else:
                trace.append("refract")
                res = sm.direct_refraction(S, rng, obj, src, out, sm.normal(S, obj, src, out, trace, g), g, k, trace)
                if res is None:
                    trace.append("refract-open")
                    return np.zeros(3)
                L, nxt = res
        elif S.reflex[obj] == 0:
            trace.append("diffuse")
            L, nxt = sm.diffuse_like(S, rng, obj, src, out, sm.normal(S, obj, src, out, trace, g), g, fr, fr, float(k), trace)
        else:
            trace.append("mirror")
            L, nxt = sm.mirror(S, rng, obj, src, out, sm.normal(S, obj, src, out, trace, g), g, fr, k, trace)
        if nxt is None:
            break
        push_dir, rate, obj, src, out = nxt
        stack.append((push_dir, rate))
    for d, r in reversed(stack):
        L = L * r + d
    return L


def sample(S, x, y, width, height, eye, cam, frame, trace=None):
    """One sample of pixel (x, y) of a textured render: smooth_spec.sample's camera ray and pixel assembly."""
    rng = jade_spec.wang_stream(x, y, frame)
    trace = trace if trace is not None else []
    lx = (-1 + 2.0 / width * (x + next(rng) - 0.5)) * (width / height)
    ly = -1 + 2.0 / height * (y + next(rng) - 0.5)
    M = np.asarray(cam, np.float64).reshape(4, 4)
    v = np.array([lx, ly, -1.5, 0.0])
    d = np.array([sum(M[c][r] * v[c] for c in range(4)) for r in range(3)])
    d = d / math.sqrt(d @ d)
    o = np.asarray(eye, np.float64)
    h, hp = S.hit(o, d, -1)
    if h < 0:
        trace.append("sky")
        return S.sky(d)
    return S.emis[h] + path_tracing(S, rng, h, hp, -d, trace)
