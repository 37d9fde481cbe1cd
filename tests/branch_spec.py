"""Stratified branch draws (include/jade_bvh.h, "The branch draws, stated"; jade_scene_set_branch_sampling = JADE_BRANCH_STRATIFIED) in
numpy, written from the header's text and NOT from csrc/jade_shade.h: integers for A, B, D and U (uint32, wrapping), float32 for su and
the comparisons.

A(i), B(i), D(x, y, frame, d), U(x, y, frame, sidx, d) and su(W) take arrays.  decisions(U, refract) says which arm a vertex takes.
sample(...): jade_spec.sample's loop with the named draws replaced - the first select, the SSS select and the mirror's roulette of the
vertices of depth 0 and 1 read U; the stream makes its draws all the same and they are dropped - and everything else an arm's own:
ARMS names the estimators the mode is built with (the reference's, the cosine bounce through bounce_spec, MIS through mis_spec, and the
environment mixture through env_mixture_spec).  The stream is seeded frame + sidx; the numbers are formed from frame and sidx.  The trace
gets, beside the arm's tags: branch-d0 / branch-d1 (a vertex that read dimension A / B), branch-free (a vertex of depth >= 2), and
sss-d0 / sss-d1, bssrdf-d0 / bssrdf-d1, mirror-d0 / mirror-d1: the arm a vertex took on that dimension's number."""
import math

import numpy as np

import bounce_spec
import env_mixture_spec
import jade_spec
import mis_spec
from jade_spec import PI, RR, SSS

U32 = np.uint32
F32 = np.float32
SALT = (0x68E31DA4, 0xB5297A4D)


def A(i):
    """The bit reversal of i: van der Corput in base 2 as 32-bit fixed point."""
    i = np.asarray(i, np.uint64) & np.uint64(0xffffffff)
    r = np.zeros_like(i)
    for b in range(32):
        r |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    return r.astype(U32)


def B(i):
    """Sobol's second dimension: r = 0; v = 0x80000000; for every bit of i, lowest first: if (i & 1) r ^= v; i >>= 1; v ^= v >> 1."""
    i = np.asarray(i, np.uint64) & np.uint64(0xffffffff)
    r = np.zeros_like(i)
    v = 0x80000000
    for b in range(32):
        r ^= ((i >> np.uint64(b)) & np.uint64(1)) * np.uint64(v)
        v ^= v >> 1
    return r.astype(U32)


def wang(s):
    """jade_wang (include/jade_fpmath.h) on uint64 arrays holding uint32 values: the next state, which is also the draw."""
    m = np.uint64(0xffffffff)
    s = (s ^ np.uint64(61)) ^ (s >> np.uint64(16))
    s = (s * np.uint64(9)) & m
    s = s ^ (s >> np.uint64(4))
    s = (s * np.uint64(0x27d4eb2d)) & m
    return s ^ (s >> np.uint64(15))


def D(x, y, frame, d):
    """The shift of a pixel's render for dimension d: jade_rng_seed(x, y, frame) ^ salt[d], then jade_wang twice; the second result."""
    m = np.uint64(0xffffffff)
    x, y, frame = (np.asarray(v, np.uint64) & m for v in (x, y, frame))
    d = np.asarray(d)
    seed = ((x * np.uint64(1973) + y * np.uint64(9277) + frame * np.uint64(26699)) & m) | np.uint64(1)
    s = seed ^ np.where(d == 0, np.uint64(SALT[0]), np.uint64(SALT[1]))
    return wang(wang(s)).astype(U32)


def U(x, y, frame, sidx, d):
    """The stratified number of sample sidx of pixel (x, y) at a vertex of depth d (0 or 1)."""
    d = np.asarray(d)
    assert ((d == 0) | (d == 1)).all()
    return np.where(d == 0, A(sidx), B(sidx)).astype(U32) ^ D(x, y, frame, d)


def shl1(W):
    """V = U << 1, wrapping."""
    return ((np.asarray(W, np.uint64) << np.uint64(1)) & np.uint64(0xffffffff)).astype(U32)


def su(W):
    """jade_rand's own conversion: (float)W * 2^-32, in float32."""
    return np.asarray(W, U32).astype(F32) * F32(2.3283064365386963e-10)


def decisions(W, refract, sss_rate=SSS, rr_rate=RR):
    """What a vertex of depth < 2 with number W decides, as bool arrays: (refraction arm, SSS-diffuse of it, the mirror's roulette goes
    on).  refract: the material has a refraction arm.  The comparisons are float32 against the fp32 constants."""
    W = np.asarray(W, U32)
    arm = (su(W) < F32(0.5)) & refract
    later = su(shl1(W)) if refract else su(W)
    return arm, later < F32(sss_rate), later < F32(rr_rate)


def mirror(S, rng, obj, src, out, n, fr, k, rr):
    """jade_spec.mirror with the roulette's number given: the stream's draw is made and dropped."""
    next(rng)
    if not rr < RR:
        return np.zeros(3), None
    r = n * (2 * (out @ n)) - out
    kk = k / (RR / PI)
    h, hp = S.hit(src, r, obj)
    if h >= 0:
        return np.zeros(3), (np.zeros(3), fr * kk, h, hp, -r)
    return S.sky(r) * fr * kk, None


# an arm: (Scene, diffuse_like, bssrdf, diffuse_like takes sss=)
def _mixture_scene(bounce, direct_mis):
    return env_mixture_spec.Arm(bounce, direct_mis).Scene


ARMS = {
    "reference": (jade_spec.Scene, jade_spec.diffuse_like, jade_spec.bssrdf, False),
    "cosine": (bounce_spec.Scene, bounce_spec.diffuse_like, bounce_spec.bssrdf, False),
    "mis": (mis_spec.Scene, mis_spec.diffuse_like, bounce_spec.bssrdf, True),
    "mixture": (_mixture_scene(env_mixture_spec.UNIFORM, False), env_mixture_spec.diffuse_like, env_mixture_spec.bssrdf, True),
}


def scene(arm, hs, env_sampling=0, light_sampling=0):
    return ARMS[arm][0](hs, env_sampling, light_sampling)


def path_tracing(S, rng, obj, src, out, trace, number, arm, stratified=True):
    """jade_spec.path_tracing's loop.  number(d): U at depth d.  stratified=False: the stream's own draws everywhere (the random mode)."""
    _, diffuse_like, bssrdf, takes_sss = ARMS[arm]
    stack = []
    L = np.zeros(3)
    while len(stack) < 128:
        if jade_spec.emissive(S, obj, 1.4e-5):
            L = S.emis[obj].copy()
            break
        L = np.zeros(3)
        n = S.norm[obj]
        fr = S.brdf[obj] * float(F32(1.0 / PI))
        refract = S.refract[obj] != 0
        k = 2 if refract else 1
        d = len(stack)
        strat = stratified and d < 2
        u = next(rng)
        W = None
        if strat:
            trace.append(f"branch-d{d}")
            W = number(d)
            u = float(su(W))
        else:
            trace.append("branch-free")
        V = (shl1(W) if refract else W) if strat else None
        if u < 0.5 and refract:
            if S.refract[obj] == 1:
                u2 = next(rng)
                if strat:
                    u2 = float(su(V))
                if strat:
                    trace.append(f"sss-d{d}" if u2 < SSS else f"bssrdf-d{d}")
                if u2 < SSS:
                    trace.append("sss")
                    fa = S.albedo[obj] * float(F32(1.0 / PI))
                    kw = dict(sss=True) if takes_sss else {}
                    L, nxt = diffuse_like(S, rng, obj, src, out, n, fa, fr, k / SSS, trace, **kw)
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
            if strat:
                trace.append(f"mirror-d{d}")
                L, nxt = mirror(S, rng, obj, src, out, n, fr, k, float(su(V)))
            else:
                L, nxt = jade_spec.mirror(S, rng, obj, src, out, n, fr, k)
        if nxt is None:
            break
        push_dir, rate, obj, src, out = nxt
        stack.append((push_dir, rate))
    for dd, r in reversed(stack):
        L = L * r + dd
    return L


def sample(S, x, y, width, height, eye, cam, frame, sidx, trace=None, arm="reference", stratified=True):
    """Sample sidx of pixel (x, y) of a render with `frame`: jade_spec.sample's camera ray and pixel assembly."""
    rng = jade_spec.wang_stream(x, y, frame + sidx)
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
    number = lambda depth: U(x, y, frame, sidx, depth)[()]
    L = S.emis[h] + path_tracing(S, rng, h, hp, -d, trace, number, arm, stratified)
    if "mix-ambiguous" in trace and "bssrdf-coplanar" not in trace:
        trace.append("bssrdf-coplanar")
    return L


# ------------------------------------------------------------------------------------------------------------------ the rows --

def rows():
    """uint32 [k, 5] rows (x, y, frame, sidx, depth) the number is checked on: sidx 0 .. 4095, 2^k and 2^k +- 1 up to 2^31, and 2^32 - 1;
    x, y in {0, 1, 15, 16, 1919, 65535}; several frames; depth 0 and 1."""
    sidx = list(range(4096))
    for k in range(32):
        sidx += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    sidx.append(2 ** 32 - 1)
    sidx = np.unique(np.array(sidx, np.uint64) & np.uint64(0xffffffff)).astype(U32)
    xs = np.array([0, 1, 15, 16, 1919, 65535], U32)
    frames = np.array([0, 1, 7, 1000, 0x7fffffff, 0xffffffff], U32)
    out = []
    # every sidx at every depth on a few pixels and frames ...
    for x, y, f in ((0, 0, 0), (1919, 1, 7), (65535, 65535, 0xffffffff), (15, 16, 1000)):
        for d in (0, 1):
            r = np.zeros((len(sidx), 5), U32)
            r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4] = x, y, f, sidx, d
            out.append(r)
    # ... and every pixel pair, frame and depth on a few of them
    few = np.array([0, 1, 2, 3, 5, 64, 4095, 2 ** 31, 2 ** 32 - 1], np.uint64).astype(U32)
    g = np.array([(x, y, f, s, d) for x in xs for y in xs for f in frames for s in few for d in (0, 1)], np.uint64).astype(U32)
    out.append(g)
    return np.ascontiguousarray(np.concatenate(out))


def number_rows(r):
    r = np.asarray(r, U32)
    return U(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4])


def is_net(a, b, k):
    """Whether the 2^k points (a, b) (uint32 each) form a (0, k, 2)-net in base 2: every elementary interval 2^-j x 2^-(k-j) holds
    exactly one point."""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    assert len(a) == len(b) == 1 << k
    for j in range(k + 1):
        cell = ((a >> np.uint64(32 - j)) if j else np.zeros_like(a)) << np.uint64(k - j)
        cell = cell | ((b >> np.uint64(32 - (k - j))) if k - j else np.zeros_like(b))
        if len(np.unique(cell)) != 1 << k:
            return False
    return True
