"""Cosine-weighted bounce sampling (include/jade_bvh.h, "The bounce, stated"; jade_scene_set_bounce_sampling = JADE_BOUNCE_COSINE) in
float64 numpy, written from the header's text and NOT from csrc/jade_shade.h.

draw(n, s, u1, u2): the direction of one draw.  The discrete decisions are taken on the fp32 inputs - the fallback predicate (on nn formed
in fp32 as the header forms it), sg (the sign of s * n.z; -0 counts as >= 0) and s - and everything else is float64.

sample(...): jade_spec.sample with the diffuse / SSS-diffuse and the BSSRDF branch restated for the mode; jade_spec.Scene, direct_diffuse,
direct_bssrdf, mirror, direct_refraction, env_draw and light_draw are jade_spec's own.  The trace gets, beside jade_spec's tags:
cos-env (an environment ray drawn by this mode), cos-indirect (an indirect ray drawn by it), cos-fallback (a vertex whose normal gave no
axis: the reference's direction and weights) and cos-nonunit (an axis from a normal with |nn - 1| > 1e-3)."""
import math

import numpy as np

import jade_spec
from jade_spec import PI, RR, SSS

F32 = np.float32


def nn_f32(n):
    """dot(n, n) as the header forms it: fma(n.z, n.z, fma(n.y, n.y, n.x * n.x)), each step rounded once.  A float64 product of two
    floats is exact and the sum of two such is rounded to fp32 once: that is the fma.  Rows [k, 3] -> [k] float32."""
    n = np.asarray(n, F32).reshape(-1, 3).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (n[:, 0] * n[:, 0]).astype(F32)
        t = (n[:, 1] * n[:, 1] + t.astype(np.float64)).astype(F32)
        return (n[:, 2] * n[:, 2] + t.astype(np.float64)).astype(F32)


def falls_back(n):
    nn = nn_f32(n)
    with np.errstate(invalid="ignore"):
        return ~((nn > 0) & (nn < np.inf))


def sphere_dir_at(u1, u2):
    """The reference's sphere direction on two given uniforms (jade_spec.sphere_dir's statements): rows [k, 3]."""
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    c = 2 * (u1 - 0.5)
    s = np.sqrt(1 - c * c)
    phi = 2 * PI * u2
    return np.stack([s * np.cos(phi), s * np.sin(phi), c], -1)


def frame(a):
    """The branchless frame about unit rows a [k, 3] (float64), sg taken from the sign bit rule of the header: (t, b)."""
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    sg = np.where(az >= 0, 1.0, -1.0)          # (-0.0 >= 0 is true)
    p = -1.0 / (sg + az)
    q = ax * ay * p
    t = np.stack([1 + sg * ax * ax * p, sg * q, -sg * ax], -1)
    b = np.stack([q, sg + ay * ay * p, -ay], -1)
    return t, b


def axis(n, s):
    """a = s * n / |n| in float64 from fp32 rows n and s = +-1, with sg's decision taken on the fp32 inputs: where n.z is +-0 the
    component is +0 (so that -0 counts as >= 0 whatever s is)."""
    n64 = np.asarray(n, F32).reshape(-1, 3).astype(np.float64)
    s = np.where(np.asarray(s, F32).reshape(-1) < 0, -1.0, 1.0)
    with np.errstate(all="ignore"):
        a = s[:, None] * n64 / np.sqrt((n64 * n64).sum(-1))[:, None]
    a[:, 2] = np.where(n64[:, 2] == 0, 0.0, a[:, 2])
    return a


def draw(n, s, u1, u2):
    """Rows n [k, 3], s [k] (+-1), u1, u2 [k] (fp32 values) -> (d [k, 3] float64, fallback [k] bool, cz [k]).
    A fallback row is the reference's sphere direction on (u1, u2), negated where dot(d, n) * s < 0; its cz is NaN."""
    n = np.asarray(n, F32).reshape(-1, 3)
    k = len(n)
    s = np.broadcast_to(np.asarray(s, F32).reshape(-1), (k,))
    u1 = np.broadcast_to(np.asarray(u1, F32).reshape(-1), (k,)).astype(np.float64)
    u2 = np.broadcast_to(np.asarray(u2, F32).reshape(-1), (k,)).astype(np.float64)
    fb = falls_back(n)
    with np.errstate(all="ignore"):
        a = axis(n, s)
        t, b = frame(a)
        r, cz = np.sqrt(u1), np.sqrt(1 - u1)
        phi = (2 * PI * u2).astype(F32).astype(np.float64)       # the double product rounded to float
        d = t * (r * np.cos(phi))[:, None] + b * (r * np.sin(phi))[:, None] + a * cz[:, None]
        c = 2 * (u1 - 0.5)
        ref = np.stack([np.sqrt(1 - c * c) * np.cos(phi), np.sqrt(1 - c * c) * np.sin(phi), c], -1)
        flip =(ref * n.astype(np.float64)).sum(-1) * s.astype(np.float64) < 0
    ref = np.where(flip[:, None], -ref, ref)
    d = np.where(fb[:, None], ref, d)
    return d, fb, np.where(fb, np.nan, cz)


U1_EDGES = np.array([0, 2.0 ** -32, 2.0 ** -24, 0.25, 0.5, 1 - 2.0 ** -24, 1.0], F32)
U2_EDGES = np.array([0, 0.25, 0.5, 0.75, 1 - 2.0 ** -24, 1.0], F32)


def normal_sets():
    """(normals that give an axis, normals that do not) - fp32 rows.  The scales are powers of two (and 2.5, 1e-3) under which nn is a
    finite positive number, 0 or inf by orders of magnitude: the predicate does not depend on rounding or on the order of the sum."""
    rng = np.random.default_rng(2017)
    v = rng.normal(size=(64, 3))
    unit = (v / np.sqrt((v * v).sum(-1))[:, None]).astype(F32)
    tiny = np.float32(2.0 ** -149)
    ok = [np.eye(3, dtype=F32), -np.eye(3, dtype=F32),
          np.array([[0.6, 0.8, 0.0], [0.6, 0.8, -0.0], [1, 0, 0.0], [1, 0, -0.0]], F32),
          np.array([[x, y, k * tiny] for x, y in ((0.6, 0.8), (1, 0)) for k in (1, 2, -1, -2)], F32),     # a.z within 2 ulp of 0
          unit, unit * F32(2.5), unit * F32(1e-3), unit * F32(2.0 ** -60), unit * F32(2.0 ** 60)]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    with np.errstate(over="ignore"):
        none = [np.zeros((1, 3), F32), np.array([[nan, 0.5, 0.5], [0.5, nan, 0.5], [0.5, 0.5, nan]], F32),
                np.array([[inf, 0.5, 0.5], [0.5, -inf, 0.5], [0.5, 0.5, inf], [-inf, 0, 0]], F32),
                unit[:8] * F32(2.0 ** -80), unit[:8] * F32(2.0 ** 70)]
    return np.concatenate(ok), np.concatenate(none)


def rows():
    """The rows (n[3], s, u1, u2) the draw is checked on, fp32 [k, 6]: every normal of normal_sets under s = +-1 with every pair of
    (U1_EDGES, U2_EDGES), then 4 096 random rows whose uniforms are (float)uint32 * 2^-32 as jade_rand forms them."""
    ok, none = normal_sets()
    alln = np.concatenate([ok, none])
    grid = np.array([(s, a, b) for s in (1.0, -1.0) for a in U1_EDGES for b in U2_EDGES], F32)
    edge = np.concatenate([np.repeat(alln, len(grid), 0), np.tile(grid, (len(alln), 1))], 1)
    rng = np.random.default_rng(950)
    k = 4096
    u = (rng.integers(0, 2 ** 32, size=(k, 2), dtype=np.uint64).astype(F32) * F32(2.0 ** -32)).astype(F32)
    n = alln[rng.integers(0, len(alln), size=k)]
    s = np.where(rng.random(k) < 0.5, F32(-1), F32(1)).astype(F32)
    return np.concatenate([edge, np.concatenate([n, s[:, None], u], 1)]).astype(F32)


def draw1(n, s, u1, u2):
    d, fb, cz = draw(np.asarray(n, F32)[None], [s], [u1], [u2])
    return d[0], bool(fb[0]), float(cz[0])


def weight(n, d, fb):
    """What the mode multiplies with where the reference has |dot(n, d)|: sqrt(nn) / 2, the reference's own on a fallback vertex."""
    n = np.asarray(n, np.float64)
    return abs(n @ d) if fb else math.sqrt(n @ n) / 2


def bounce_dir(rng, n32, side, ref_flip, trace, tag):
    """One ray of the mode at a vertex with stored normal n32 (fp32): s = -1 iff side < 0.  On a fallback the direction is the
    reference's, flipped by the reference's own test ref_flip(w)."""
    u1, u2 = next(rng), next(rng)
    s = -1.0 if side < 0 else 1.0
    if bool(falls_back(n32)[0]):
        trace.append("cos-fallback")
        w = sphere_dir_at(u1, u2)
        return (-w if ref_flip(w) else w), True
    trace.append(tag)
    if abs(float(nn_f32(n32)[0]) - 1) > 1e-3:
        trace.append("cos-nonunit")
    d, fb, _ = draw1(n32, s, u1, u2)
    assert not fb
    return d, False


def diffuse_like(S, rng, obj, src, out, n, f, fr, scale, trace):
    """jade_spec.diffuse_like under JADE_BOUNCE_COSINE."""
    n32 = S.norm32[obj]
    side = out @ n
    flip = lambda w: (w @ n) * side < 0
    L = jade_spec.direct_diffuse(S, rng, obj, src, n, side, f, trace)
    if S.env_sampling:                                   # the environment ray stays the importance draw, with its own weight
        w, ratio = S.env_draw(rng)
        if (w @ n) * side < 0:
            trace.append("env-noenv")
        else:
            trace.append("env-importance")
            h, _ = S.hit(src, w, obj)
            if h < 0:
                L = L + S.sky(w) * f * abs(n @ w) * 2 * PI * ratio
    else:
        w, fb = bounce_dir(rng, n32, side, flip, trace, "cos-env")
        h, _ = S.hit(src, w, obj)
        if h < 0:
            L = L + S.sky(w) * f * weight(n, w, fb) * 2 * PI
    L = L * scale
    if not next(rng) < RR:
        return L, None
    w, fb = bounce_dir(rng, n32, side, flip, trace, "cos-indirect")
    h, hp = S.hit(src, w, obj)
    if h >= 0 and not jade_spec.emissive_ge(S, h):
        w = -w
        rate = fr * weight(n, w, fb) / RR * scale
        return L, (L, rate, h, hp, w)
    return L, None


def bssrdf(S, rng, obj, src, out, n, k, trace):
    """jade_spec.bssrdf under JADE_BOUNCE_COSINE (the exit search, the profile and the emitters are restated word for word)."""
    seg = S.segs[S.obj[obj]]
    A = S.prefix[seg[1]]
    xi = next(rng) * A
    left, right, mid = int(seg[0]), int(seg[1]), 0
    while left < right - 1:
        mid = (left + right) // 2
        if xi <= S.prefix[mid]:
            right = mid
        elif xi >= S.prefix[mid]:
            left = mid
        else:
            break
    m = int(S.mapping[mid])
    rx, ry = next(rng), next(rng)
    Q = S.point(m, rx, ry)
    inner = Q - src
    r = math.sqrt(inner @ inner)
    d = S.rate[m]
    Rd = (np.exp(-r / d) + np.exp(-r / 3.0 / d)) / (d * (8 * PI * r))
    eta = S.eta[m]
    R0 = ((eta - 1) / (eta + 1)) ** 2
    Fi = R0 + (1 - R0) * (1 - abs(n @ out)) ** 5
    Rd = Rd * Fi
    nm, nm32 = S.norm[m], S.norm32[m]
    Aobj = S.prefix[S.segs[S.obj[m]][1]]
    if abs(inner @ nm) < 1e-5 * r * math.sqrt(nm @ nm):
        trace.append("bssrdf-coplanar")

    def Fo(v):
        return R0 - (1 - R0) * (1 - abs(v @ nm)) ** 5

    L = jade_spec.direct_bssrdf(S, rng, Q, m, nm, Rd, Fo, Aobj, trace)
    inn = inner @ nm
    if S.env_sampling:
        w, ratio = S.env_draw(rng)
        if (w @ nm) * inn < 0:
            trace.append("env-noenv")
        else:
            trace.append("env-importance")
            h, _ = S.hit(Q, w, m)
            if h < 0:
                L = L + S.sky(w) * Fo(w) * Rd * abs(nm @ w) * 2 * ratio
    else:
        w, fb = bounce_dir(rng, nm32, inn, lambda v: (v @ nm) * inn < 0, trace, "cos-env")
        h, _ = S.hit(Q, w, m)
        if h < 0:
            L = L + S.sky(w) * Fo(w) * Rd * weight(nm, w, fb) * 2
    L = L * (k / (1 - SSS))
    # drawn BEFORE the roulette draw; the OPPOSITE hemisphere: s = -1 iff dot(inner, t_norm) > 0
    w, fb = bounce_dir(rng, nm32, -inn, lambda v: (v @ nm) * inn > 0, trace, "cos-indirect")
    if not next(rng) < RR:
        return L, None
    h, hp = S.hit(Q, w, m)
    if h >= 0 and not jade_spec.emissive_ge(S, h):
        w = -w
        rate = Rd * Fo(w) * weight(nm, w, fb) * Aobj * 2 / RR * (k / (1 - SSS))
        return L, (L, rate, h, hp, w)
    return L, None


class Scene(jade_spec.Scene):
    """jade_spec.Scene plus the normals as stored (fp32): the mode's discrete decisions are taken on them."""

    def __init__(self, hs, env_sampling=0, light_sampling=0):
        super().__init__(hs, env_sampling, light_sampling)
        self.norm32 = hs.a["triangles"].view(F32)[:, 10:13].copy()


def path_tracing(S, rng, obj, src, out, trace):
    """jade_spec.path_tracing's loop with the two branches above."""
    stack = []
    L = np.zeros(3)
    while len(stack) < 128:
        if jade_spec.emissive(S, obj, 1.4e-5):
            L = S.emis[obj].copy()
            break
        L = np.zeros(3)
        n = S.norm[obj]
        fr = S.brdf[obj] * float(F32(1.0 / PI))
        k = 2 if S.refract[obj] != 0 else 1
        u = next(rng)
        if u < 0.5 and S.refract[obj] != 0:
            if S.refract[obj] == 1:
                if next(rng) < SSS:
                    trace.append("sss")
                    fa = S.albedo[obj] * float(F32(1.0 / PI))
                    L, nxt = diffuse_like(S, rng, obj, src, out, n, fa, fr, k / SSS, trace)
                else:
                    trace.append("bssrdf")
                    L, nxt = bssrdf(S, rng, obj, src, out, n, k, trace)
            else:
                trace.append("refract")
                res = jade_spec.direct_refraction(S, rng, obj, src, out, n, k, None)
                if res is None:
                    trace.append("refract-open")
                    return np.zeros(3)
                L, nxt = res
        elif S.reflex[obj] == 0:
            trace.append("diffuse")
            L, nxt = diffuse_like(S, rng, obj, src, out, n, fr, fr, float(k), trace)
        else:
            trace.append("mirror")
            L, nxt = jade_spec.mirror(S, rng, obj, src, out, n, fr, k)
        if nxt is None:
            break
        push_dir, rate, obj, src, out = nxt
        stack.append((push_dir, rate))
    for d, r in reversed(stack):
        L = L * r + d
    return L


def sample(S, x, y, width, height, eye, cam, frame, trace=None):
    """One sample of pixel (x, y) under JADE_BOUNCE_COSINE: jade_spec.sample's camera ray and pixel assembly."""
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
