"""Multiple importance sampling of the emitters (include/jade_bvh.h, "The direct light, stated"; jade_scene_set_direct_sampling =
JADE_DIRECT_MIS, on top of JADE_BOUNCE_COSINE) in float64 numpy, written from the header's text and NOT from csrc/jade_shade.h or
jade_scene_prep.hip.

table(tf, emit, light_table): the two numbers (m, M) per triangle.  The discrete decisions - the emission threshold, the area and the
normal's squared length being finite and positive - are taken on the fp32 values as the header forms them; M is rounded to fp32 once.
densities / w_emitter / g_bounce: the two densities and what each side makes of them, in float64, written as two code paths - the
emitter side as 1 / (1 + pB / PL), the bounce side as m |n.omega| sqrt(nne) / (PL + pB) - so that a test can hold their sum to 1.
sample(...): bounce_spec.sample with the diffuse / SSS-diffuse branch restated for the mode; the BSSRDF branch, mirror, refraction,
the draws and the scene are bounce_spec's and jade_spec's own.  The trace gets, beside theirs: mis-weighted (an emitter term that took
a weight), mis-unweighted (one that did not: its triangle is not weighted, or the vertex fell back), mis-bounce-lit (T_B added),
mis-bounce-unlisted (the indirect ray ended on an emitting triangle that is not weighted: nothing added) and mis-sss-bounce-lit (T_B
added at an SSS-diffuse vertex, with refract_albedo / pi)."""
import math

import numpy as np

import bounce_spec
import jade_spec
import lights_spec
from bounce_spec import bounce_dir, falls_back, nn_f32, weight
from jade_spec import PI, RR, SSS

F32 = np.float32
PI32 = float(F32(PI))        # fl(pi) of the reference's 3.1415926


def weighted(tf):
    """[n] bool: the triangle rows tf [n, 28] (fp32) that are WEIGHTED - not all channels < 1.5e-4f, area and dot(ne, ne) finite and > 0."""
    tf = np.asarray(tf, F32)
    with np.errstate(all="ignore"):
        emits = ~(tf[:, 13:16] < F32(1.5e-4)).all(1)
        a = lights_spec.tri_size_f32(tf)
        nne = nn_f32(tf[:, 10:13])
        return emits & (a > 0) & np.isfinite(a) & (nne > 0) & np.isfinite(nne)


def table(tf, emit, light_table=None):
    """(m [n], M [n]) float64 of the triangle rows tf under the list emit.  light_table: JADE_LIGHTS_ONE's table over emit (lights_spec.TABLE
    records; which entry is paired with which is not part of any statement, so the table is data) or None: M = 0."""
    tf = np.asarray(tf, F32)
    emit = np.asarray(emit, np.int64)
    n, nE = len(tf), len(emit)
    count = np.bincount(emit, minlength=n).astype(np.float64) if nE else np.zeros(n)
    prob = np.zeros(n)
    if light_table is not None and nE:
        assert len(light_table) == nE
        for i in range(nE):                                   # in list order, in double
            prob[emit[i]] += float(light_table["q_own"][i])
        prob = (prob / float(nE)).astype(F32).astype(np.float64)
    w = weighted(tf)
    return np.where(w, count, 0.0), np.where(w, prob, 0.0)


def densities(n, ne, A, mu, l):
    """(PL, pB) per solid angle at a vertex of stored normal n, towards the point at l on a triangle of stored normal ne and area A."""
    with np.errstate(all="ignore"):
        ll = l @ l
        rl = math.sqrt(ll)
        pA = np.float64(ll * rl * math.sqrt(ne @ ne)) / np.float64(A * abs(ne @ l))
        pB = np.float64(abs(n @ l)) / np.float64(rl * math.sqrt(n @ n) * PI32)
        return mu * pA, pB


def applies(n32, m):
    """The mode does something at this vertex for this triangle: the triangle is weighted and the normal gives the cosine draw an axis."""
    return bool(m > 0) and not bool(falls_back(np.asarray(n32, F32))[0])


def w_emitter(n32, ne, A, m, mu, l):
    """What an emitter term towards the triangle is multiplied with (the emitter side's code path)."""
    if not applies(n32, m):
        return 1.0
    PL, pB = densities(np.asarray(n32, np.float64), ne, A, mu, l)
    with np.errstate(all="ignore"):
        return float(1.0 / (1.0 + pB / PL))


def g_bounce(n32, ne, A, m, mu, l):
    """The scalar factor of the bounce term, T_B = Le f g_B / RR (the bounce side's code path)."""
    if not applies(n32, m):
        return 0.0
    n = np.asarray(n32, np.float64)
    PL, pB = densities(n, ne, A, mu, l)
    with np.errstate(all="ignore"):
        return float(np.float64(m * (abs(n @ l) / math.sqrt(l @ l)) * math.sqrt(ne @ ne)) / (PL + pB))


def terms_rows(rows):
    """Rows (n[3], ne[3], A, m, mu, l[3], Le, f), fp32 [k, 14] -> (w_L [k], T_B [k]) float64, T_B = Le f g_B / fl(0.9): what
    jade_debug_mis_terms returns."""
    rows = np.asarray(rows, F32)
    r = rows.astype(np.float64)
    w = np.array([w_emitter(rows[i, 0:3], r[i, 3:6], r[i, 6], r[i, 7], r[i, 8], r[i, 9:12]) for i in range(len(r))])
    g = np.array([g_bounce(rows[i, 0:3], r[i, 3:6], r[i, 6], r[i, 7], r[i, 8], r[i, 9:12]) for i in range(len(r))])
    with np.errstate(all="ignore"):
        return w, r[:, 12] * r[:, 13] * g / float(F32(0.9))


class Scene(bounce_spec.Scene):
    """bounce_spec.Scene plus the table: m per triangle, and mu = m with all lights, M with one."""

    def __init__(self, hs, env_sampling=0, light_sampling=0):
        super().__init__(hs, env_sampling, light_sampling)
        tf = hs.a["triangles"].view(F32)
        self.mis_m, M = table(tf, self.emit, self.light_table if light_sampling else None)
        self.mis_mu = M if light_sampling else self.mis_m


def emitter_term(S, obj, src, n, f, e, l, weight_, trace):
    """One entry's term (jade_spec.direct_diffuse's, times the one-light weight) times w_L."""
    ll = l @ l
    term = S.emis[e] * f * abs((n @ l) * (S.norm[e] @ l)) / ll / ll * S.area(e) * weight_
    if applies(S.norm32[obj], S.mis_m[e]):
        trace.append("mis-weighted")
    else:
        trace.append("mis-unweighted")
    return term * w_emitter(S.norm32[obj], S.norm[e], S.area(e), S.mis_m[e], S.mis_mu[e], l)


def direct_diffuse(S, rng, obj, src, n, side, f, trace):
    """jade_spec.direct_diffuse with every found entry's term weighed."""
    L = np.zeros(3)
    if S.light_sampling:
        if len(S.emit) == 0:
            return L
        e, P, wt = jade_spec.light_draw(S, rng, trace)
        l = P - src
        if (l @ n) * side < 0:
            trace.append("light-side")
            return L
        h, _ = S.hit(src, l, obj)
        if h != e:
            trace.append("light-shadowed")
            return L
        jade_spec.light_found(S, e, wt, trace)
        return L + emitter_term(S, obj, src, n, f, e, l, wt, trace)
    for e in S.emit:
        rx, ry = jade_spec.light_uniforms(rng, 2)
        l = S.point(e, rx, ry) - src
        if (l @ n) * side < 0:
            continue
        h, _ = S.hit(src, l, obj)
        if h == e:
            L = L + emitter_term(S, obj, src, n, f, e, l, 1.0, trace)
    return L


def bounce_term(S, obj, src, f, h, hp, sss, trace):
    """T_B for an indirect ray from the vertex on obj at src whose nearest hit is h at hp; zero where h is not weighted."""
    if not applies(S.norm32[obj], S.mis_m[h]):
        if jade_spec.emissive_ge(S, h):
            trace.append("mis-bounce-unlisted")
        return np.zeros(3)
    trace.append("mis-sss-bounce-lit" if sss else "mis-bounce-lit")
    g = g_bounce(S.norm32[obj], S.norm[h], S.area(h), S.mis_m[h], S.mis_mu[h], hp - src)
    return S.emis[h] * f * g / RR


def diffuse_like(S, rng, obj, src, out, n, f, fr, scale, trace, sss=False):
    """bounce_spec.diffuse_like under JADE_DIRECT_MIS: the roulette and the indirect ray are drawn where they were; what the indirect
    ray finds is looked at BEFORE the scale, because the bounce term is part of l_dir."""
    n32 = S.norm32[obj]
    side = out @ n
    flip = lambda w: (w @ n) * side < 0
    L = direct_diffuse(S, rng, obj, src, n, side, f, trace)
    if S.env_sampling:
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
    if not next(rng) < RR:
        return L * scale, None
    w, fb = bounce_dir(rng, n32, side, flip, trace, "cos-indirect")
    h, hp = S.hit(src, w, obj)
    if h >= 0:
        L = L + bounce_term(S, obj, src, f, h, hp, sss, trace)
    L = L * scale
    if h >= 0 and not jade_spec.emissive_ge(S, h):
        w = -w
        rate = fr * weight(n, w, fb) / RR * scale
        return L, (L, rate, h, hp, w)
    return L, None


def path_tracing(S, rng, obj, src, out, trace):
    """bounce_spec.path_tracing's loop with the diffuse / SSS-diffuse branch above."""
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
                    L, nxt = diffuse_like(S, rng, obj, src, out, n, fa, fr, k / SSS, trace, sss=True)
                else:
                    trace.append("bssrdf")
                    L, nxt = bounce_spec.bssrdf(S, rng, obj, src, out, n, k, trace)
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
    """One sample of pixel (x, y) under JADE_DIRECT_MIS: jade_spec.sample's camera ray and pixel assembly."""
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


def table_of(lib, tf, emit):
    """jade_debug_mis_table_host (libjade_hip_debug.so; no HIP call) on triangle rows tf [n, 28] and emit [nE]: (m [n], M [n]) float32."""
    import ctypes as C
    fn = lib.jade_debug_mis_table_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    tf = np.ascontiguousarray(tf, F32)
    assert tf.shape[1] == 28
    emit = np.ascontiguousarray(emit, np.int32)
    out = np.full((len(tf), 2), np.nan, F32)
    rc = fn(tf.ctypes.data, len(tf), emit.ctypes.data if len(emit) else None, len(emit), out.ctypes.data)
    assert rc == 0, rc
    return out[:, 0], out[:, 1]
