"""Smooth shading (include/jade_bvh.h, "The shading normal, stated"; jade_scene_set_vertex_normals) in float64 numpy, written from the
header's text and NOT from csrc/jade_smooth.h or jade_smooth_shade.h.

normal_rows(rows): the function of (triangle, point, reference direction) on rows of 27 fp32 numbers - p1 p2 p3 n1 n2 n3 g p r.  The discrete
decisions are taken on the fp32 inputs - FLAT (the three normals bitwise g), DEGENERATE (N.N, formed in double from the fp32 corners as
the header forms it), the sum's predicate (bounce_spec.falls_back on the sum rounded to fp32) - and everything else is float64.  Beside
the normal and the rule it returns the row's error bound D and whether the side rule's two products clear it.

sample(...): jade_spec.sample with EVERY branch restated for the mode - mirror, diffuse, SSS-diffuse, BSSRDF, the refraction entry and its
loop - under the reference estimator, JADE_BOUNCE_COSINE and JADE_ENV_IMPORTANCE.  The trace gets, beside jade_spec's and bounce_spec's tags:
smooth (a vertex that used the interpolated normal), smooth-flat (one that took g because its triangle is flat or degenerate or its sum
has no direction), smooth-side (one that took g by the side rule), smooth-redirect (a mirror or refraction direction formed again with
g), smooth-culled (a drawn direction that passed the test against n and failed it against g) and smooth-undecided (a side product of any
of these tests within its bound of 0: the fp32 render may decide it either way)."""
import math

import numpy as np

import bounce_spec
import jade_spec
from jade_spec import PI, RR, SSS

F32 = np.float32
E = 2.0 ** -24
RULE_NS, RULE_FLAT, RULE_DEGENERATE, RULE_SUM, RULE_SIDE = 0, 1, 2, 3, 4
# The bound on a side product in the render (sample): the unit vectors it is formed from carry the error of the fp32 vertex, not of one
# function.  A hit point is off by a few ulp of its coordinates (|x| <= 3 in these scenes: ~5e-7), the dual vectors of an edge of length l
# turn that into 5e-7 / l of a barycentric (l >= 0.3 on the ball: 2e-6), times |n_i - n_1| <= 0.4: 1e-6 of ns, and `out` is a normalised
# fp32 direction (2e-7).  A product of unit vectors within 1e-5 of 0 - three times that sum - is left undecided; jade_spec's
# bssrdf-coplanar uses the same figure for the same reason.
SIDE_EPS = 1e-5


def _unit_len(v):
    return np.sqrt((v * v).sum(-1))


def duals(p1, p2, p3):
    """(d2, d3, NN) in float64 from float64 copies of the fp32 corners, rows [k, 3]."""
    e1, e2 = p2 - p1, p3 - p1
    N = np.cross(e1, e2)
    NN = (N * N).sum(-1)
    with np.errstate(all="ignore"):
        return np.cross(e2, N) / NN[:, None], np.cross(N, e1) / NN[:, None], NN


def normal_rows(rows):
    """rows fp32 [k, 27] -> dict(n [k, 3] float64, rule [k], D [k] the bound on a component of n where rule is RULE_NS, clear [k] bool:
    the side rule's products are further from 0 than their error, ns [k, 3] the interpolated unit normal (NaN where there is none))."""
    rows = np.asarray(rows, F32).reshape(-1, 27)
    r64 = rows.astype(np.float64)
    p1, p2, p3, n1, n2, n3, g, p, r = (r64[:, 3 * i:3 * i + 3] for i in range(9))
    k = len(rows)
    bits = rows.view(np.uint32)
    flat = np.ones(k, bool)
    for i in (3, 4, 5):
        flat &= (bits[:, 3 * i:3 * i + 3] == bits[:, 18:21]).all(-1)
    d2, d3, NN = duals(p1, p2, p3)
    with np.errstate(all="ignore"):
        degenerate = ~((NN > 0) & (NN < np.inf))
        w = p - p1
        b2, b3 = (w * d2).sum(-1), (w * d3).sum(-1)
        s = (1 - b2 - b3)[:, None] * n1 + b2[:, None] * n2 + b3[:, None] * n3
        nosum = bounce_spec.falls_back(s.astype(F32))
        ln = _unit_len(s)
        ns = s / ln[:, None]
        a, b = (ns * r).sum(-1), (g * r).sum(-1)
        side = ~(((a > 0) & (b > 0)) | ((a < 0) & (b < 0)))
        # the bound (tests/test_gpu_smooth.py derives it): errors of b2, b3, then of the sum, then of the normalised sum
        lw, lr, lg = _unit_len(w), _unit_len(r), _unit_len(g)
        m2, m3 = _unit_len(n2 - n1), _unit_len(n3 - n1)
        eb2, eb3 = 6 * E * lw * _unit_len(d2), 6 * E * lw * _unit_len(d3)
        es = eb2 * m2 + eb3 * m3 + 4 * E * (_unit_len(n1) + np.abs(b2) * m2 + np.abs(b3) * m3)
        D = 2 * es / ln + 4 * E
        clear = (np.abs(a) > (np.sqrt(3.0) * D + 4 * E) * lr) & (np.abs(b) > 4 * E * lg * lr)
    rule = np.where(flat, RULE_FLAT, np.where(degenerate, RULE_DEGENERATE, np.where(nosum, RULE_SUM, np.where(side, RULE_SIDE, RULE_NS))))
    n = np.where((rule == RULE_NS)[:, None], ns, g)
    return dict(n=n, rule=rule, D=D, clear=clear | (rule < RULE_SIDE) & (rule > RULE_NS), ns=ns)


def special_rows():
    """The rows whose rule does not depend on rounding: a degenerate triangle (two corners equal; three in a line), zero / NaN / inf
    normals, a flat-marked triangle, r in the plane of g (g.r = 0 exactly) and r = 0."""
    tri = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    up = [0, 0, 1]
    tilt = [0.6, 0, 0.8, 0, 0.6, 0.8, -0.6, 0, 0.8]
    p = [0.25, 0.25, 0]
    nan, inf = float("nan"), float("inf")
    rows = [
        [0, 0, 0, 0, 0, 0, 0, 1, 0] + tilt + up + p + [0, 0, 1],          # p2 = p1
        [0, 0, 0, 1, 1, 0, 2, 2, 0] + tilt + up + p + [0, 0, 1],          # three in a line
        tri + [0] * 9 + up + p + [0, 0, 1],                                # zero normals: the sum is 0
        tri + [nan, 0, 1] + tilt[3:] + up + p + [0, 0, 1],
        tri + tilt[:6] + [0, inf, 1] + up + p + [0, 0, 1],
        tri + [1e30, 0, 1e30] * 3 + up + p + [0, 0, 1],                    # the sum's square overflows fp32
        tri + up * 3 + up + p + [0.3, 0.2, 1],                             # flat-marked
        tri + up * 3 + up + p + [0.3, 0.2, -1],
        tri + tilt + up + p + [1, 0, 0],                                   # r in the plane of g
        tri + tilt + up + p + [0, 0, 0],                                   # no direction at all
        tri + tilt + up + p + [0, 0, 1],                                   # ... and the plain case beside them
        tri + tilt + up + p + [0, 0, -1],
        tri + tilt + up + p + [-0.9, 0, 0.1],                              # ns.r < 0 < g.r: the side rule (ns = (0, .., ..) leaning to +x at p)
    ]
    return np.array(rows, F32)


def random_rows(k, seed=950):
    """Random triangles (edges 0.05 .. 2, no slivers: the smallest angle is above ~6 degrees), unit corner normals within ~50 degrees of
    g on either side of it, points inside and up to 5 % outside, r anywhere - a quarter of them near the plane of g or of ns so that the
    side rule fires."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((0, 27), F32)
    while len(rows) < k:
        m = 2 * (k - len(rows)) + 64
        p1 = rng.uniform(-3, 3, (m, 3))
        e1 = rng.normal(size=(m, 3))
        e1 *= (rng.uniform(0.05, 2, m) / _unit_len(e1))[:, None]
        e2 = rng.normal(size=(m, 3))
        e2 *= (rng.uniform(0.05, 2, m) / _unit_len(e2))[:, None]
        N = np.cross(e1, e2)
        sin = _unit_len(N) / (_unit_len(e1) * _unit_len(e2))
        g = N / _unit_len(N)[:, None]
        g = g * np.where(rng.random(m) < 0.5, -1.0, 1.0)[:, None]
        nn = [g + 0.6 * rng.normal(size=(m, 3)) * rng.random((m, 1)) for _ in range(3)]
        nn = [v / _unit_len(v)[:, None] for v in nn]
        b = rng.dirichlet((1, 1, 1), m) * 1.1 - 0.05
        b[:, 0] = 1 - b[:, 1] - b[:, 2]
        p = p1 + b[:, 1:2] * e1 + b[:, 2:3] * e2
        r = rng.normal(size=(m, 3))
        graze = rng.random(m) < 0.25
        r = np.where(graze[:, None], r - (r * g).sum(-1)[:, None] * g * rng.uniform(0.7, 1.3, (m, 1)), r)
        block = np.concatenate([p1, p1 + e1, p1 + e2] + nn + [g, p, r], 1).astype(F32)
        rows = np.concatenate([rows, block[sin > 0.1]])
    return rows[:k]


# ------------------------------------------------------------------------------------------------------------ the arm of jade_spec.sample --
class Scene(bounce_spec.Scene):
    """bounce_spec.Scene plus the host scene's vertex normals (fp32 [n, 3, 3]; None: every triangle is flat) and the bounce sampling."""

    def __init__(self, hs, env_sampling=0, light_sampling=0, cosine=False):
        assert not light_sampling, "smooth shading is not built with JADE_LIGHTS_ONE"
        super().__init__(hs, env_sampling, 0)
        self.cosine = cosine
        t = hs.a["triangles"].view(F32)
        vn = hs.vertex_normals
        if vn is None:
            vn = np.repeat(t[:, None, 10:13], 3, 1)
        self.vn32 = np.ascontiguousarray(vn, F32).reshape(-1, 9)
        self.tri32 = np.ascontiguousarray(t[:, 1:13])          # p1 p2 p3 g


def normal(S, k, p, r, trace, g=None):
    """normal(triangle k, p, r) of the header -> the vertex's normal (float64); tags the trace.  Where the answer is the flat normal it is
    the very object g (S.norm[k] if none is given): the tests below against g are then the tests against n over again, and are not made twice."""
    row = np.concatenate([S.tri32[k, :9], S.vn32[k], S.tri32[k, 9:12], np.zeros(6, F32)]).astype(F32)
    out = normal_rows(row[None])       # FLAT / DEGENERATE / the sum's predicate: on the fp32 inputs; p and r are float64 below
    g = S.norm[k] if g is None else g
    if out["rule"][0] in (RULE_FLAT, RULE_DEGENERATE):
        trace.append("smooth-flat")
        return g
    d2, d3, _ = duals(S.p1[k][None], S.p2[k][None], S.p3[k][None])
    w = p - S.p1[k]
    b2, b3 = float(w @ d2[0]), float(w @ d3[0])
    n1, n2, n3 = (S.vn32[k, 3 * i:3 * i + 3].astype(np.float64) for i in range(3))
    s = (1 - b2 - b3) * n1 + b2 * n2 + b3 * n3
    if bool(bounce_spec.falls_back(s.astype(F32))[0]):
        trace.append("smooth-flat")
        return g
    ns = s / math.sqrt(s @ s)
    a, b = ns @ r, g @ r
    lr = math.sqrt(r @ r)
    if abs(a) <= SIDE_EPS * lr or abs(b) <= SIDE_EPS * lr * math.sqrt(g @ g):
        trace.append("smooth-undecided")
    if not ((a > 0 and b > 0) or (a < 0 and b < 0)):
        trace.append("smooth-side")
        return g
    trace.append("smooth")
    return ns


def _sides(d, r, g, trace):
    """(dot(d, g), dot(r, g)); tags smooth-undecided where either is within the bound of 0."""
    x, y = d @ g, r @ g
    lg = math.sqrt(g @ g)
    if abs(x) <= SIDE_EPS * lg * math.sqrt(d @ d) or abs(y) <= SIDE_EPS * lg * math.sqrt(r @ r):
        trace.append("smooth-undecided")
    return x, y


def same(d, r, g, trace, n=None):
    if n is g:
        return True                 # formed with g itself: the reflection of r about the plane of g lies on r's side
    x, y = _sides(d, r, g, trace)
    return (x > 0 and y > 0) or (x < 0 and y < 0)


def other(d, r, g, trace, n=None):
    if n is g:
        return True                 # formed with g itself: a refracted (or totally reflected, unchanged) direction crosses the plane of g
    x, y = _sides(d, r, g, trace)
    return (x > 0 and y < 0) or (x < 0 and y > 0)


def culled(d, ref, g, trace, opposite=False, n=None):
    """The test against g of a drawn direction that passed the test against n: dot(d, g) * dot(ref, g) < 0 (> 0 for the BSSRDF indirect ray).
    Where n is g it is the test the direction has just passed."""
    if n is g:
        return False
    x, y = _sides(d, ref, g, trace)
    out = x * y > 0 if opposite else x * y < 0
    if out:
        trace.append("smooth-culled")
    return out


def mirror(S, rng, obj, src, out, n, g, fr, k, trace):
    if not next(rng) < RR:
        return np.zeros(3), None
    r = n * (2 * (out @ n)) - out
    if not same(r, out, g, trace, n):
        trace.append("smooth-redirect")
        r = g * (2 * (out @ g)) - out
    kk = k / (RR / PI)
    h, hp = S.hit(src, r, obj)
    if h >= 0:
        return np.zeros(3), (np.zeros(3), fr * kk, h, hp, -r)
    return S.sky(r) * fr * kk, None


def hemisphere(S, rng, n, n32ish, side, flip, trace, tag):
    """One drawn direction about normal n (float64; the cosine draw takes it rounded to fp32, as the render holds it) and whether the
    vertex fell back to the reference's weight."""
    if S.cosine:
        return bounce_spec.bounce_dir(rng, n32ish, side, flip, trace, tag)
    w = jade_spec.sphere_dir(rng)
    return (-w if flip(w) else w), True


def weight(S, n, d, fb):
    return abs(n @ d) if (fb or not S.cosine) else math.sqrt(n @ n) / 2


def diffuse_like(S, rng, obj, src, out, n, g, f, fr, scale, trace):
    side, side_g = out @ n, out @ g
    n32 = n.astype(F32)[None]
    flip = lambda w: (w @ n) * side < 0
    L = np.zeros(3)
    for e in S.emit:
        rx, ry = jade_spec.light_uniforms(rng, 2)
        l = S.point(e, rx, ry) - src
        if (l @ n) * side < 0:
            continue
        if culled(l, out, g, trace, n=n):
            continue
        h, _ = S.hit(src, l, obj)
        if h == e:
            ll = l @ l
            L = L + S.emis[e] * f * abs((n @ l) * (S.norm[e] @ l)) / ll / ll * S.area(e)
    if S.env_sampling:
        w, ratio = S.env_draw(rng)
        if (w @ n) * side < 0:
            trace.append("env-noenv")
        elif not culled(w, out, g, trace, n=n):
            trace.append("env-importance")
            h, _ = S.hit(src, w, obj)
            if h < 0:
                L = L + S.sky(w) * f * abs(n @ w) * 2 * PI * ratio
    else:
        w, fb = hemisphere(S, rng, n, n32, side, flip, trace, "cos-env")
        if not culled(w, out, g, trace, n=n):
            h, _ = S.hit(src, w, obj)
            if h < 0:
                L = L + S.sky(w) * f * weight(S, n, w, fb) * 2 * PI
    L = L * scale
    if not next(rng) < RR:
        return L, None
    w, fb = hemisphere(S, rng, n, n32, side, flip, trace, "cos-indirect")
    if culled(w, out, g, trace, n=n):
        return L, None
    h, hp = S.hit(src, w, obj)
    if h >= 0 and not jade_spec.emissive_ge(S, h):
        w = -w
        rate = fr * weight(S, n, w, fb) / RR * scale
        return L, (L, rate, h, hp, w)
    return L, None


def bssrdf(S, rng, obj, src, out, n, k, trace):
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
    gm = S.norm[m]
    if abs(inner @ gm) < 1e-5 * r * math.sqrt(gm @ gm):
        trace.append("bssrdf-coplanar")
    nm = normal(S, m, Q, inner, trace, gm)
    nm32 = nm.astype(F32)[None]
    Aobj = S.prefix[S.segs[S.obj[m]][1]]

    def Fo(v):
        return R0 - (1 - R0) * (1 - abs(v @ nm)) ** 5

    L = np.zeros(3)
    for e in S.emit:                             # no side test in this branch, against either normal
        ex, ey = jade_spec.light_uniforms(rng, 2)
        l = S.point(e, ex, ey) - Q
        h, _ = S.hit(Q, l, m)
        if h == e:
            ll = l @ l
            L = L + S.emis[e] * Fo(l / math.sqrt(ll)) * Rd * abs((nm @ l) * (S.norm[e] @ l)) / ll / ll * S.area(e) / PI * Aobj
    inn = inner @ nm
    if S.env_sampling:
        w, ratio = S.env_draw(rng)
        if (w @ nm) * inn < 0:
            trace.append("env-noenv")
        elif not culled(w, inner, gm, trace, n=nm):
            trace.append("env-importance")
            h, _ = S.hit(Q, w, m)
            if h < 0:
                L = L + S.sky(w) * Fo(w) * Rd * abs(nm @ w) * 2 * ratio
    else:
        w, fb = hemisphere(S, rng, nm, nm32, inn, lambda v: (v @ nm) * inn < 0, trace, "cos-env")
        if not culled(w, inner, gm, trace, n=nm):
            h, _ = S.hit(Q, w, m)
            if h < 0:
                L = L + S.sky(w) * Fo(w) * Rd * weight(S, nm, w, fb) * 2
    L = L * (k / (1 - SSS))
    w, fb = hemisphere(S, rng, nm, nm32, -inn, lambda v: (v @ nm) * inn > 0, trace, "cos-indirect")   # drawn BEFORE the roulette draw
    if not next(rng) < RR:
        return L, None
    if culled(w, inner, gm, trace, opposite=True, n=nm):
        return L, None
    h, hp = S.hit(Q, w, m)
    if h >= 0 and not jade_spec.emissive_ge(S, h):
        w = -w
        rate = Rd * Fo(w) * weight(S, nm, w, fb) * Aobj * 2 / RR * (k / (1 - SSS))
        return L, (L, rate, h, hp, w)
    return L, None


def direct_refraction(S, rng, obj, src, out, n, g, k, trace):
    eta = S.eta[obj]
    R0 = ((1 - eta) / (1 + eta)) ** 2
    t, _ = jade_spec.refract(-out, n, float(F32(1.0 / eta)))
    nn = n
    if not other(t, out, g, trace, n):
        trace.append("smooth-redirect")
        nn = g
        t, _ = jade_spec.refract(-out, g, float(F32(1.0 / eta)))
    Fi = R0 + (1 - R0) * (1 - abs(nn @ out)) ** 5
    rate = np.full(3, 1 - Fi)
    origin, prev = src, obj
    for _ in range(32):
        h, hp = S.hit(origin, t, prev)
        if h < 0:
            return None
        gh = S.norm[h]
        rev = -t
        seg = origin - hp
        rate = rate * S.rate[h] ** math.sqrt(seg @ seg)
        origin, prev = hp, h
        u = next(rng)

        def form(hn):
            d, tir = jade_spec.refract(t, hn, eta)
            Fo = R0 - (1 - R0) * (1 - abs(d @ hn)) ** 5
            reflected = tir or u < 0.2
            if reflected:
                d = d - hn * (2 * (d @ hn))
            return d, tir, Fo, reflected

        nh = normal(S, h, hp, rev, trace, gh)
        d, tir, Fo, reflected = form(nh)
        if not (same(d, rev, gh, trace, nh) if reflected else other(d, rev, gh, trace, nh)):
            trace.append("smooth-redirect")
            d, tir, Fo, reflected = form(gh)
        t = d
        if reflected:
            if not tir:
                rate = rate * (Fo * 5)
        else:
            rate = rate * ((1.0 - Fo) * 1.25)
            break
    if not next(rng) < RR:
        return np.zeros(3), None
    h, hp = S.hit(origin, t, prev)
    if h >= 0:
        return np.zeros(3), (np.zeros(3), rate * (k / RR), h, hp, -t)
    return S.sky(t) * rate * (k / RR), None


def path_tracing(S, rng, obj, src, out, trace):
    """jade_spec.path_tracing's loop with every branch above."""
    stack = []
    L = np.zeros(3)
    while len(stack) < 128:
        if jade_spec.emissive(S, obj, 1.4e-5):
            L = S.emis[obj].copy()
            break
        L = np.zeros(3)
        g = S.norm[obj]
        fr = S.brdf[obj] * float(F32(1.0 / PI))
        k = 2 if S.refract[obj] != 0 else 1
        u = next(rng)
        if u < 0.5 and S.refract[obj] != 0:
            if S.refract[obj] == 1:
                if next(rng) < SSS:
                    trace.append("sss")
                    fa = S.albedo[obj] * float(F32(1.0 / PI))
                    L, nxt = diffuse_like(S, rng, obj, src, out, normal(S, obj, src, out, trace, g), g, fa, fr, k / SSS, trace)
                else:
                    trace.append("bssrdf")
                    L, nxt = bssrdf(S, rng, obj, src, out, normal(S, obj, src, out, trace, g), k, trace)
            else:
                trace.append("refract")
                res = direct_refraction(S, rng, obj, src, out, normal(S, obj, src, out, trace, g), g, k, trace)
                if res is None:
                    trace.append("refract-open")
                    return np.zeros(3)
                L, nxt = res
        elif S.reflex[obj] == 0:
            trace.append("diffuse")
            L, nxt = diffuse_like(S, rng, obj, src, out, normal(S, obj, src, out, trace, g), g, fr, fr, float(k), trace)
        else:
            trace.append("mirror")
            L, nxt = mirror(S, rng, obj, src, out, normal(S, obj, src, out, trace, g), g, fr, k, trace)
        if nxt is None:
            break
        push_dir, rate, obj, src, out = nxt
        stack.append((push_dir, rate))
    for d, r in reversed(stack):
        L = L * r + d
    return L


def sample(S, x, y, width, height, eye, cam, frame, trace=None):
    """One sample of pixel (x, y) of a smooth render: jade_spec.sample's camera ray and pixel assembly."""
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
