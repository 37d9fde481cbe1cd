"""Normal maps (include/jade_bvh.h, "The mapped normal, stated"; jade_scene_set_normal_maps) in float64 numpy, written from the header's
text and NOT from csrc/jade_normal_map.h or the kernels.  Built on texture_spec (uv, the fetch) and smooth_spec (normal(), ns, the side rule).

frame_rows(corners, uv6): the record's T, B and whether the triangle is UNMAPPED, in float64 from the fp32 corners and the fp32 du2, du3.
mapped_rows(rows, images, image, strength): normal'(triangle, p, r) on rows of 33 fp32 numbers - p1 p2 p3 n1 n2 n3 g uv1 uv2 uv3 p r - with the
rule, the row's error bound D on a component of the result, and whether a decision of the cascade lies within its bound of a branch
(undecided: the fp32 device may take either).  mapped_rows32: the per-vertex arithmetic of a MAPPED row in emulated fp32, op for op.
sample(...): texture_spec.sample with normal' wherever the arm asks for the normal.  Tags beside smooth_spec's and texture_spec's: mapped (a
vertex that used the bent normal), mapped-zero (step 5), mapped-side (step 8 fell back to normal()), mapped-culled (a drawn direction that
passed the test against a bent normal and failed it against g).

The bound D of a MAPPED row, e = 2^-24, per component (mapped_rows forms it from the row's float64 quantities):
  m: the device's fp32 (u, v) is within (D_u, D_v) of the statement's (texture_spec.uv_rows) and the fetch is piecewise linear with slope at
  most W step per unit of u and H step per unit of v: (D_u W + D_v H) step, plus the fetch's own roundings (texture_spec.fetch_roundings):
  D_m.  mx = fl(strength m.x): strength D_m + e |mx|.
  nb: ns carries smooth_spec.normal_rows' D; g / sqrt(g.g) three roundings of a unit vector's component, 4 e.
  T, B: unit vectors rounded once, e each.
  t = fma(mz, nb, fma(my, B, fl(mx T))): |nb_c|, |T_c|, |B_c| <= 1, so  D_t = D_m (1 + 2 strength) + |mz| D_nb + 2 e (|mx| + |my|) + 3 e (|mx| +
  |my| + |mz|) - the inputs' errors, the frame's roundings, the three operations' roundings of numbers no larger than |mx| + |my| + |mz|.
  nm = t / sqrt(tt): a vector off by d, normalised, is off by at most 2 |d| / |t|, |d| <= sqrt(3) D_t; the dot, the root and the division
  round: D = 2 sqrt(3) D_t / |t| + 4 e.
  The side rule's a = dot(nm, r) is then within (sqrt(3) D + 4 e) |r| of its float64 value and b = dot(g, r) within 4 e |g| |r| (as in
  smooth_spec); mx and my are within strength D_m + e |mx| of theirs."""
import contextlib
import math

import numpy as np

import bounce_spec
import smooth_spec
import texture_spec
from texture_spec import E, F32, dot32, fetch32, fetch64, fma32

RULE_MAPPED, RULE_MAP_ZERO, RULE_MAP_SUM, RULE_MAP_SIDE_NS = 5, 6, 7, 8
ROW = 33


def _len(v):
    return np.sqrt((v * v).sum(-1))


def _in_range(x):
    with np.errstate(all="ignore"):
        return (x > 0) & (x < np.inf)


def frame_rows(corners, uv6):
    """corners fp32 [k, 9] (p1 p2 p3), uv6 fp32 [k, 6] -> (T [k, 3], B [k, 3] float64 unit vectors, unmapped [k]): the record's frame."""
    c = np.asarray(corners, F32).reshape(-1, 9).astype(np.float64)
    uv = np.asarray(uv6, F32).reshape(-1, 6)
    with np.errstate(all="ignore"):
        du2 = (uv[:, 2:4] - uv[:, 0:2]).astype(np.float64)           # one fp32 subtraction per component, as the record holds them
        du3 = (uv[:, 4:6] - uv[:, 0:2]).astype(np.float64)
        e1, e2 = c[:, 3:6] - c[:, 0:3], c[:, 6:9] - c[:, 0:3]
        N = np.cross(e1, e2)
        NN = (N * N).sum(-1)
        det = du2[:, 0] * du3[:, 1] - du3[:, 0] * du2[:, 1]
        T = (e1 * du3[:, 1:2] - e2 * du2[:, 1:2]) / det[:, None]
        B = (e2 * du2[:, 0:1] - e1 * du3[:, 0:1]) / det[:, None]
        lt, lb = _len(T), _len(B)
        unmapped = ~_in_range(NN) | (det == 0) | ~np.isfinite(det) | ~_in_range(lt) | ~_in_range(lb)
        T, B = T / lt[:, None], B / lb[:, None]
    return T, B, unmapped


def _split(rows):
    rows = np.asarray(rows, F32).reshape(-1, ROW)
    rows27 = np.concatenate([rows[:, 0:21], rows[:, 27:33]], 1)                 # smooth_spec's: p1 p2 p3 n1 n2 n3 g p r
    rows18 = np.concatenate([rows[:, 0:9], rows[:, 21:27], rows[:, 27:30]], 1)  # texture_spec's: p1 p2 p3 uv1 uv2 uv3 p
    return rows, rows27, rows18


def mapped_rows(rows, images, image, strength):
    """rows fp32 [k, 33]; images: a list of fp32 [H, W, 3]; image int [k] (-1: none); strength: a float (taken as fp32) -> dict(n [k, 3]
    float64, rule [k], D [k], undecided [k] bool, nm [k, 3] the bent normal where one is formed (NaN elsewhere) with its bound Dnm, ns [k, 3]
    the interpolated normal with its bound Dns: the candidates an undecided row's answer is one of, beside g)."""
    rows, rows27, rows18 = _split(rows)
    k = len(rows)
    image = np.asarray(image, np.int64).reshape(k)
    s = float(F32(strength))
    sm = smooth_spec.normal_rows(rows27)
    T, B, unmapped = frame_rows(rows[:, 0:9], rows[:, 21:27])
    unmapped = unmapped | (image < 0)
    uvr = texture_spec.uv_rows(rows18)
    r64 = rows.astype(np.float64)
    g, r = r64[:, 18:21], r64[:, 30:33]
    with np.errstate(all="ignore"):
        uv_ok = np.isfinite(uvr["uv"]).all(1)
        m = np.full((k, 3), np.nan)
        Dm = np.zeros(k)
        flat0 = np.zeros(k, bool)                                     # every tap of the row has x = y = 0 exactly: the tilt is 0 in any arithmetic
        for i, im in enumerate(images):
            sel = (image == i) & ~unmapped & uv_ok
            if not sel.any():
                continue
            H, W = im.shape[:2]
            m[sel] = fetch64(im, uvr["uv"][sel, 0], uvr["uv"][sel, 1])
            Dm[sel] = (uvr["D"][sel, 0] * W + uvr["D"][sel, 1] * H) * texture_spec.texel_step(im) + texture_spec.fetch_roundings(im)
            tilt = np.abs(np.asarray(im, np.float64)[..., 0:2]).sum(-1, keepdims=True) * np.ones(3)
            flat0[sel] = fetch64(tilt, uvr["uv"][sel, 0], uvr["uv"][sel, 1])[:, 0] == 0
        fetched = ~unmapped & uv_ok
        mx, my, mz = s * m[:, 0], s * m[:, 1], m[:, 2]
        Dxy = s * Dm + E * np.maximum(np.abs(mx), np.abs(my))
        zero = fetched & (((mx == 0) & (my == 0)) | np.isnan(mx) | np.isnan(my) | np.isnan(mz))
        near_zero = fetched & ~flat0 & (s != 0) & (np.abs(mx) <= Dxy) & (np.abs(my) <= Dxy)     # (a strength of 0 is a tilt of 0 in any arithmetic)
        # the base: ns before its side rule where the triangle is ON and its sum has a direction, else g / |g|
        on = (sm["rule"] == smooth_spec.RULE_NS) | (sm["rule"] == smooth_spec.RULE_SIDE)
        gg32 = dot32(rows[:, 18:21], rows[:, 18:21])
        g_ok = _in_range(gg32.astype(np.float64))
        nb = np.where(on[:, None], sm["ns"], g / _len(g)[:, None])
        Dnb = np.where(on, sm["D"], 4 * E)
        have = on | g_ok
        t = mz[:, None] * nb + my[:, None] * B + mx[:, None] * T
        nosum = bounce_spec.falls_back(np.where(np.isfinite(t), t, np.nan).astype(F32)) | ~np.isfinite(t).all(1)
        lt = _len(t)
        nm = t / lt[:, None]
        mag = np.abs(mx) + np.abs(my) + np.abs(mz)
        Dt = Dm * (1 + 2 * s) + np.abs(mz) * Dnb + 2 * E * (np.abs(mx) + np.abs(my)) + 3 * E * mag
        D = 2 * math.sqrt(3.0) * Dt / lt + 4 * E
        a, b = (nm * r).sum(-1), (g * r).sum(-1)
        lr, lg = _len(r), _len(g)
        right = ((a > 0) & (b > 0)) | ((a < 0) & (b < 0))
        clear = (np.abs(a) > (math.sqrt(3.0) * D + 4 * E) * lr) & (np.abs(b) > 4 * E * lg * lr)
    formed = fetched & ~zero & have & ~nosum
    mapped = formed & right
    rule = np.where(mapped, RULE_MAPPED, sm["rule"])
    rule = np.where(fetched & zero, RULE_MAP_ZERO, rule)
    rule = np.where(fetched & ~zero & (~have | nosum), RULE_MAP_SUM, rule)
    rule = np.where(formed & ~right & (sm["rule"] == smooth_spec.RULE_NS), RULE_MAP_SIDE_NS, rule)
    n = np.where(mapped[:, None], nm, sm["n"])
    Dout = np.where(mapped, D, sm["D"])
    # undecided: the tilt within its bound of zero; the bent normal's side within its bound; and where normal() answers, its own side rule
    undecided = near_zero | (formed & ~clear) | (~mapped & ~sm["clear"])
    return dict(n=n, rule=rule, D=Dout, undecided=undecided, nm=np.where(formed[:, None], nm, np.nan), Dnm=D, ns=sm["ns"], Dns=sm["D"], Dm=Dm, m=m)


def mapped_rows32(rows, images, image, strength):
    """The statement's fp32 operations from the record to nm on every row (float32 [k, 3]; meaningful where mapped_rows' rule is RULE_MAPPED):
    the record's d2, d3, T, B formed in double and rounded once, then uv, the fetch, the base, the sum and the normalisation op for op."""
    rows, rows27, rows18 = _split(rows)
    k = len(rows)
    image = np.asarray(image, np.int64).reshape(k)
    s = F32(strength)
    T, B, _ = frame_rows(rows[:, 0:9], rows[:, 21:27])
    T, B = T.astype(F32), B.astype(F32)
    uv = texture_spec.uv_rows32(rows18)
    m = np.full((k, 3), np.nan, F32)
    for i, im in enumerate(images):
        sel = image == i
        if sel.any():
            m[sel] = fetch32(im, uv[sel, 0], uv[sel, 1])
    r = rows.astype(np.float64)
    d2, d3, NN = smooth_spec.duals(r[:, 0:3], r[:, 3:6], r[:, 6:9])
    sm = smooth_spec.normal_rows(rows27)
    on = (sm["rule"] == smooth_spec.RULE_NS) | (sm["rule"] == smooth_spec.RULE_SIDE)
    with np.errstate(all="ignore"):
        d2, d3 = d2.astype(F32), d3.astype(F32)
        w = rows[:, 27:30] - rows[:, 0:3]
        b2, b3 = dot32(w, d2), dot32(w, d3)
        n1, m2, m3 = rows[:, 9:12], rows[:, 12:15] - rows[:, 9:12], rows[:, 15:18] - rows[:, 9:12]
        sv = np.stack([fma32(b3, m3[:, c], fma32(b2, m2[:, c], n1[:, c])) for c in range(3)], 1)
        ns = (sv / np.sqrt(dot32(sv, sv))[:, None]).astype(F32)
        g = rows[:, 18:21]
        gn = (g / np.sqrt(dot32(g, g))[:, None]).astype(F32)
        nb = np.where(on[:, None], ns, gn).astype(F32)
        mx, my, mz = (s * m[:, 0]).astype(F32), (s * m[:, 1]).astype(F32), m[:, 2]
        t = np.stack([fma32(mz, nb[:, c], fma32(my, B[:, c], (mx * T[:, c]).astype(F32))) for c in range(3)], 1)
        return (t / np.sqrt(dot32(t, t))[:, None]).astype(F32)


def random_rows(k, seed=961):
    """smooth_spec.random_rows' triangles, normals, points and directions with corner UVs in [-2, 3]; a third of the triangles FLAT (the
    three normals bitwise g)."""
    base = smooth_spec.random_rows(k, seed)
    rng = np.random.default_rng(seed + 1)
    flat = rng.random(k) < 1 / 3
    for i in (9, 12, 15):
        base[flat, i:i + 3] = base[flat, 18:21]
    uv = rng.uniform(-2, 3, (k, 6)).astype(F32)
    return np.concatenate([base[:, 0:21], uv, base[:, 21:27]], 1).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ the render --
ZERO_EPS = 1e-5      # a tilt this small is left undecided in the render: smooth_spec.SIDE_EPS, for the same reason


class Scene(texture_spec.Scene):
    """texture_spec.Scene plus the host scene's normal maps: hs.normal_maps = (images, uv [n, 3, 2], image_of [n], strength) or None."""

    def __init__(self, hs, env_sampling=0, light_sampling=0, cosine=False):
        super().__init__(hs, env_sampling, light_sampling, cosine)
        nm = getattr(hs, "normal_maps", None)
        n = len(self.tri32)
        if nm is None:
            self.nm_images, self.nm_uv32, self.nm_image_of, self.nm_strength = [], np.zeros((n, 6), F32), np.full(n, -1, np.int64), 1.0
        else:
            self.nm_images = [np.asarray(im, F32).astype(np.float64) for im in nm[0]]
            self.nm_uv32 = np.ascontiguousarray(nm[1], F32).reshape(n, 6)
            self.nm_image_of = np.asarray(nm[2], np.int64).reshape(n).copy()
            self.nm_strength = float(F32(nm[3]))
        self.nm_T, self.nm_B, unmapped = frame_rows(self.tri32[:, :9], self.nm_uv32)
        self.nm_image_of[unmapped] = -1


_normal = smooth_spec.normal


def normal_mapped(S, k, p, r, trace, g=None):
    """normal'(triangle k, p, r) of the header in float64; tags the trace.  Falls back to smooth_spec.normal, whose answer may be the object g."""
    im = int(S.nm_image_of[k])
    if im < 0:
        return _normal(S, k, p, r, trace, g)
    gg = S.norm[k] if g is None else g
    c = S.tri32[k, :9].astype(np.float64)
    d2, d3, _ = smooth_spec.duals(c[None, 0:3], c[None, 3:6], c[None, 6:9])
    w = np.asarray(p, np.float64) - c[0:3]
    b2, b3 = float(w @ d2[0]), float(w @ d3[0])
    uvc = S.nm_uv32[k].astype(np.float64)
    uv = uvc[0:2] + b2 * (S.nm_uv32[k, 2:4] - S.nm_uv32[k, 0:2]).astype(np.float64) + b3 * (S.nm_uv32[k, 4:6] - S.nm_uv32[k, 0:2]).astype(np.float64)
    if not np.isfinite(uv).all():
        return _normal(S, k, p, r, trace, g)
    m = fetch64(S.nm_images[im], uv[0:1], uv[1:2])[0]
    mx, my, mz = S.nm_strength * m[0], S.nm_strength * m[1], m[2]
    if (mx == 0 and my == 0) or math.isnan(mx) or math.isnan(my) or math.isnan(mz):
        trace.append("mapped-zero")
        return _normal(S, k, p, r, trace, g)
    if abs(mx) <= ZERO_EPS and abs(my) <= ZERO_EPS:
        trace.append("smooth-undecided")
    row = np.concatenate([S.tri32[k, :9], S.vn32[k], S.tri32[k, 9:12], np.zeros(6, F32)]).astype(F32)
    rule = smooth_spec.normal_rows(row[None])["rule"][0]
    nb = None
    if rule not in (smooth_spec.RULE_FLAT, smooth_spec.RULE_DEGENERATE):
        n1, n2, n3 = (S.vn32[k, 3 * i:3 * i + 3].astype(np.float64) for i in range(3))
        s = (1 - b2 - b3) * n1 + b2 * n2 + b3 * n3
        if not bool(bounce_spec.falls_back(s.astype(F32))[0]):
            nb = s / math.sqrt(s @ s)
    if nb is None:
        g32 = S.tri32[k, 9:12].astype(np.float64)
        if not (g32 @ g32 > 0 and g32 @ g32 < np.inf):
            return _normal(S, k, p, r, trace, g)
        nb = g32 / math.sqrt(g32 @ g32)
    t = mz * nb + my * S.nm_B[k] + mx * S.nm_T[k]
    if bool(bounce_spec.falls_back(t.astype(F32))[0]):
        return _normal(S, k, p, r, trace, g)
    nm = t / math.sqrt(t @ t)
    a, b = nm @ r, gg @ r
    lr = math.sqrt(r @ r)
    if abs(a) <= smooth_spec.SIDE_EPS * lr or abs(b) <= smooth_spec.SIDE_EPS * lr * math.sqrt(gg @ gg):
        trace.append("smooth-undecided")
    if (a > 0 and b > 0) or (a < 0 and b < 0):
        trace.append("mapped")
        return nm
    trace.append("mapped-side")
    return _normal(S, k, p, r, trace, g)


@contextlib.contextmanager
def _the_one_call():
    """The arm reaches the normal through one call - smooth_spec.normal, from smooth_spec's own branches and from texture_spec.path_tracing;
    a mapped render answers it with normal'."""
    smooth_spec.normal = normal_mapped
    try:
        yield
    finally:
        smooth_spec.normal = _normal


def sample(S, x, y, width, height, eye, cam, frame, trace=None):
    """One sample of pixel (x, y) of a mapped render: texture_spec.sample with normal' for normal."""
    trace = trace if trace is not None else []
    with _the_one_call():
        out = texture_spec.sample(S, x, y, width, height, eye, cam, frame, trace)
    bent = False
    for tag in list(trace):                       # a cull at a vertex whose normal is the bent one
        if tag == "mapped":
            bent = True
        elif tag in ("smooth", "smooth-flat", "smooth-side"):
            bent = False
        elif tag == "smooth-culled" and bent and "mapped-culled" not in trace:
            trace.append("mapped-culled")
    return out
