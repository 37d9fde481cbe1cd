"""The environment mixture (jade_render_params.env_sampling = JADE_ENV_MIXTURE), stated independently in float64 numpy.

Written from the text of include/jade_rt.h (at JADE_ENV_MIXTURE) and from tests/env_spec.py, tests/env_importance_spec.py and
tests/bounce_spec.py - not from csrc/jade_shade.h:

  * texel_of(dirs, W, H):  the texel a direction lies in, with the coordinates (u, v) it was formed from;
  * accepts(...) / set_size(...):  the texels within delta of those coordinates - a comparison accepts any member;
  * draw(table, W, H, n, side, technique, u0..u4):  technique, texel, own, direction, m and wrong side of one draw per row;
  * densities and quadrature over the map (p_sky, p_hemi, Quadrature): what the CPU tests integrate;
  * Arm(bounce, direct_mis):  a spec for spec_scenes.compare_arm - jade_spec.sample / bounce_spec.sample / mis_spec.sample with the
    environment draw replaced, through a Scene subclass that carries the bounce and direct sampling.

Everything is float64 except the discrete decisions, which are taken on the fp32 inputs: u0 < 0.5, the slot product, own / alias, the
fallback predicate (bounce_spec.falls_back) - and the texel of a direction, which is ambiguous within delta of a cell border."""
import math

import numpy as np

import bounce_spec
import env_importance_spec as EI
import env_spec
import jade_spec
import mis_spec
from jade_spec import PI, RR, SSS

F32 = np.float32
PI_F = EI.PI_F
E = 2.0 ** -24
UNIFORM, COSINE = 0, 1  # JADE_BOUNCE_*
# The coordinate error of an fp32 evaluation of (u, v), in units of the map's extent: env_spec.tolerance's coordinate term ("a few fp32
# ulps of u, v and of atan2 / asin move the sample point by at most about 2e-7 W texels").
UV_ERR = 2e-7
# How far a device's direction may lie from this statement's, per component (tests/test_gpu_bounce.py derives both): the cosine draw ...
D_COSINE = 48 * E + 2 * 2.5e-7 + math.sqrt(2.0) * 2.0 ** -22


def d_uniform(sin):
    """... and the reference's sphere direction (sin cs, sin sn, cos) with sin = sqrt(1 - cos^2) (test_gpu_bounce.py's D_fb)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.minimum(np.sqrt(3 * E), 1.5 * E / np.asarray(sin, np.float64)) + 3 * E + 2.5e-7 + 2.0 ** -22


# How far the sky technique's direction may lie (tests/test_gpu_env_importance.py derives it: DESIGN.md section 2 item 5)
ANGLE_BOUND = 3 * E * 2 * EI.PI
SINCOS_BOUND = 2.5e-7
D_SKY = 2 * (ANGLE_BOUND + SINCOS_BOUND) + E


# ------------------------------------------------------------------------------------------------------------------- the texel --

def texel_of(dirs, w, h):
    """(texel int64 [k], u [k], v [k]): i = min(floor(u W), W - 1), j = min(floor(v H), H - 1) of env_spec.uv_of's coordinates; a
    negative product and a NaN count as 0."""
    u, v = env_spec.uv_of(dirs)
    u, v = np.where(np.isnan(u), 0.0, u), np.where(np.isnan(v), 0.0, v)
    i = np.clip(np.floor(u * w), 0, w - 1).astype(np.int64)
    j = np.clip(np.floor(v * h), 0, h - 1).astype(np.int64)
    return j * w + i, u, v


def deltas(dirs, w, h, dir_err=0.0):
    """(du, dv) in texel units: UV_ERR of the extent, plus what an error dir_err per component of a (unit) direction moves the
    coordinates by - d(atan2) <= sqrt(2) dir_err / s and d(asin) <= sqrt(3) dir_err / s with s = sqrt(x^2 + z^2), over 2 PI and PI."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    dir_err = np.broadcast_to(np.asarray(dir_err, np.float64), (len(d),))
    with np.errstate(all="ignore"):
        s = np.sqrt(d[:, 0] ** 2 + d[:, 2] ** 2) / np.sqrt((d * d).sum(1))
        du = w * (UV_ERR + np.where(dir_err > 0, math.sqrt(2.0) * dir_err / (2 * PI * s), 0.0))
        dv = h * (UV_ERR + np.where(dir_err > 0, math.sqrt(3.0) * dir_err / (PI * s), 0.0))
    return np.where(np.isnan(du), np.inf, du), np.where(np.isnan(dv), np.inf, dv)


def _axis_range(x, n, d, wraps):
    """Cells lo .. hi (inclusive, clamped) that [x - d, x + d] meets, and whether it reaches past an end of an axis that wraps."""
    lo = np.clip(np.floor(np.maximum(x - d, -1.0)), 0, n - 1).astype(np.int64)
    hi = np.clip(np.floor(np.minimum(x + d, n + 1.0)), 0, n - 1).astype(np.int64)
    return lo, hi, (wraps & (x - d < 0), wraps & (x + d >= n))


def accepts(texel, u, v, w, h, du, dv):
    """bool [k]: texel is one of the texels within (du, dv) of (u W, v H).  The column wraps at the seam (u = 0 and u = 1 are one
    meridian); the row does not."""
    texel = np.asarray(texel, np.int64)
    j, i = np.divmod(texel, w)
    ilo, ihi, (wl, wr) = _axis_range(u * w, w, du, np.ones(len(u), bool))
    jlo, jhi, _ = _axis_range(v * h, h, dv, np.zeros(len(u), bool))
    col = ((i >= ilo) & (i <= ihi)) | (wl & (i == w - 1)) | (wr & (i == 0))
    return col & (j >= jlo) & (j <= jhi) & (texel >= 0) & (texel < w * h)


def set_size(u, v, w, h, du, dv):
    """int64 [k]: how many texels accepts() takes."""
    ilo, ihi, (wl, wr) = _axis_range(u * w, w, du, np.ones(len(u), bool))
    jlo, jhi, _ = _axis_range(v * h, h, dv, np.zeros(len(u), bool))
    cols = (ihi - ilo + 1) + (wl & (ihi < w - 1)) + (wr & (ilo > 0))
    return np.minimum(cols, w) * (jhi - jlo + 1)


# -------------------------------------------------------------------------------------------------------------------- the draw --

def hemisphere(n, side, technique, u1, u2):
    """The direction the bounce sampling draws from (u1, u2) at rows (n, side): (d float64 [k, 3], fallback [k], its error bound per
    component [k], prod [k] = the product the reference's flip decided on (NaN where no flip was asked))."""
    n = np.asarray(n, F32).reshape(-1, 3)
    k = len(n)
    side = np.broadcast_to(np.asarray(side, F32).reshape(-1), (k,))
    u1 = np.broadcast_to(np.asarray(u1, F32).reshape(-1), (k,))
    u2 = np.broadcast_to(np.asarray(u2, F32).reshape(-1), (k,))
    with np.errstate(all="ignore"):
        c = 2 * (u1.astype(np.float64) - 0.5)
        sin = np.sqrt(1 - c * c)
        phi = (2 * PI * u2.astype(np.float64)).astype(F32).astype(np.float64)
        ref = np.stack([sin * np.cos(phi), sin * np.sin(phi), c], -1)
        prod = (ref * n.astype(np.float64)).sum(-1) * side.astype(np.float64)
        ref = np.where((prod < 0)[:, None], -ref, ref)
    if technique == COSINE:
        d, fb, _ = bounce_spec.draw(n, side, u1, u2)
        return (np.where(fb[:, None], ref, d), fb, np.where(fb, d_uniform(sin), D_COSINE), np.where(fb, prod, np.nan))
    return ref, np.zeros(k, bool), d_uniform(sin), prod


def weight(q, s, c, cosine_form):
    """m = (2 P s) / (q + P s), or (2 P s) / (q + 2 P s c) in the cosine form; P = fl(PI)."""
    with np.errstate(all="ignore"):
        return np.where(cosine_form, (2 * PI_F * s) / (q + 2 * PI_F * s * c), (2 * PI_F * s) / (q + PI_F * s))


def weight_bound(q, s, c, cosine_form, ds, dc, m):
    """How far an fp32 evaluation of m may lie from weight(): m rises with s and falls with c, so over the box |s' - s| <= ds,
    |c' - c| <= dc its partial derivatives 2 P q / den^2 and (2 P s)^2 / den^2 are largest at the smallest denominator; then the six
    roundings of the formula (P s, the product with c, the sum, the quotient; the doublings are exact; q is the table's own fp32
    value on both sides).  DESIGN.md 3.16 writes it out."""
    with np.errstate(all="ignore"):
        s_lo, s_hi = np.maximum(s - ds, 0.0), s + ds
        c_lo = np.maximum(np.where(cosine_form, c, 0.0) - dc, 0.0)
        den = np.where(cosine_form, q + 2 * PI_F * s_lo * c_lo, q + PI_F * s_lo)
        by_s = 2 * PI_F * q / den ** 2 * ds
        by_c = np.where(cosine_form, (2 * PI_F * s_hi) ** 2 / den ** 2 * dc, 0.0)
        return by_s + by_c + 6 * E * np.abs(m)


def draw(table, w, h, n, side, technique, u0, u1, u2, u3, u4, texel=None):
    """One draw per row.  n [k, 3], side [k] and the five uniforms are fp32 values; technique: UNIFORM or COSINE for all rows.
    texel (optional, int64 [k]): the texel a device took for a hemisphere row - q is then that texel's, if accepts() takes it (else
    the nearest texel's, and the comparison of the texel fails by itself).  Returns a dict of arrays [k]:
      hemi, own, wrong (bool); texel (the nearest); d [k, 3]; m; q, s, c, cosine_form; u, v, du, dv (hemisphere rows: the texel's
      coordinates and their delta); d_err (the bound on a device's direction, per component); m_err (on its m);
      unsure (the flip of a hemisphere row, or the wrong-side test of a sky row, was decided by a product within rounding of 0 - or by an
      infinite component of the normal times a component of the direction within its bound of 0: a hemisphere row is then held to the
      invariants only, its direction's sign being rounding's; a sky row is held to everything but its wrong-side flag, since its
      direction, texel and m do not depend on the side)."""
    n = np.asarray(n, F32).reshape(-1, 3)
    k = len(n)
    bc = lambda x: np.broadcast_to(np.asarray(x, F32).reshape(-1), (k,))
    side, u0, u1, u2, u3, u4 = (bc(x) for x in (side, u0, u1, u2, u3, u4))
    hemi = ~(u0 < F32(0.5))
    n64 = n.astype(np.float64)
    t_sky, own, d_sky, _, q_sky = EI.draw(table, w, h, u1, u2, u3, u4)
    _, s_sky = EI.direction_of(((t_sky % w) + u3.astype(np.float64)) / w, ((t_sky // w) + u4.astype(np.float64)) / h)
    d_hemi, fb, err_hemi, prod = hemisphere(n, side, technique, u1, u2)
    d = np.where(hemi[:, None], d_hemi, d_sky)
    with np.errstate(all="ignore"):
        t_near, u, v = texel_of(d_hemi, w, h)
        du, dv = deltas(d_hemi, w, h, err_hemi)
        t_hemi = t_near
        if texel is not None:
            t_hemi = np.where(accepts(texel, u, v, w, h, du, dv), np.asarray(texel, np.int64), t_near)
        q = np.where(hemi, table["q_own"][t_hemi].astype(np.float64), q_sky)
        s = np.where(hemi, np.sqrt(d[:, 0] ** 2 + d[:, 2] ** 2), s_sky)
        nn = (n64 * n64).sum(-1)
        c = np.abs((n64 * d).sum(-1)) / np.sqrt(nn)
        cosine_form = np.full(k, technique == COSINE) & ~bounce_spec.falls_back(n)
        m = weight(q, s, c, cosine_form)
        dot_side = (d_sky * n64).sum(-1) * side.astype(np.float64)
        wrong = ~hemi & (dot_side < 0)
        d_err = np.where(hemi, err_hemi, D_SKY)
        ds = np.where(hemi, math.sqrt(2.0) * d_err + 2 * E * s, ANGLE_BOUND + SINCOS_BOUND)
        dc = math.sqrt(3.0) * d_err + 4 * E
        m_err = weight_bound(q, s, c, cosine_form, ds, dc, m)
        absn = np.where(np.isfinite(n64), np.abs(n64), 0.0).sum(-1) * np.where(np.isfinite(side), np.abs(side), 1.0)
        near0 = lambda p, e: np.isfinite(p) & (absn > 0) & (np.abs(p) <= 2 * e * absn)
        # an infinite component of the normal times a component of the direction within its bound of 0 is +-inf or NaN by rounding
        # (tests/test_gpu_bounce.py's rule); any other product with an infinite factor has the sign of that component on both sides
        inf_small = (np.isinf(n64) & (np.abs(d) <= d_err[:, None])).any(-1)
        unsure = np.where(hemi, near0(prod, err_hemi) | (inf_small & (fb | (technique == UNIFORM))), near0(dot_side, D_SKY) | inf_small)
        unsure = unsure | np.isinf(side)
    return dict(hemi=hemi, own=own & ~hemi, wrong=wrong, texel=np.where(hemi, t_near, t_sky), d=d, m=m, q=q, s=s, c=c,
                cosine_form=cosine_form, u=u, v=v, du=du, dv=dv, d_err=d_err, m_err=m_err, unsure=unsure, fallback=fb)


# ------------------------------------------------------------------------------------------------------- densities, quadrature --

def p_sky(table, w, h, dirs):
    """q_t / (2 pi^2 sin theta) of the texel each unit direction lies in."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    t, _, _ = texel_of(d, w, h)
    with np.errstate(divide="ignore"):
        return table["q_own"][t].astype(np.float64) / (2 * PI * PI * np.sqrt(d[:, 0] ** 2 + d[:, 2] ** 2))


def p_hemi(n, side, technique, dirs):
    """1 / 2 pi or c / pi on the side of the surface (n, side) and 0 off it; a normal that gives no axis takes the uniform form."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    n64 = np.asarray(n, F32).astype(np.float64)
    on = (d @ n64) * float(side) >= 0
    if technique == COSINE and not bool(bounce_spec.falls_back(np.asarray(n, F32)[None])[0]):
        return np.where(on, np.abs(d @ n64) / math.sqrt(n64 @ n64) / PI, 0.0)
    return np.where(on, 1 / (2 * PI), 0.0)


class Quadrature:
    """Midpoints of a ku x kv grid in every texel of a W x H map: directions, solid-angle weights and the texel of each point.  Exact
    for what is constant per texel in (u, v) and smooth otherwise."""

    def __init__(self, w, h, ku, kv):
        self.w, self.h = w, h
        u = (np.arange(w * ku) + 0.5) / (w * ku)
        v = (np.arange(h * kv) + 0.5) / (h * kv)
        uu, vv = np.meshgrid(u, v)
        theta = PI * vv.ravel()
        phi = 2 * PI * (uu.ravel() - 0.5)
        st = np.sin(theta)
        self.d = np.stack([st * np.cos(phi), np.cos(theta), st * np.sin(phi)], -1)
        self.dw = 2 * PI * PI * st / (w * ku * h * kv)
        self.texel = (np.floor(vv.ravel() * h).astype(np.int64)) * w + np.floor(uu.ravel() * w).astype(np.int64)

    def integral(self, f):
        return float((f * self.dw).sum())


def integrand(Q, lum, n, side):
    """g = L |n.w| on the side of the surface (n, side), 0 off it, per quadrature point: the ONE environment term without its 2 pi and
    its weight, no visibility.  lum: L per quadrature point."""
    n64 = np.asarray(n, F32).astype(np.float64)
    on = (Q.d @ n64) * float(side) >= 0
    return np.where(on, lum * np.abs(Q.d @ n64), 0.0)


def densities(Q, table, n, side, technique):
    """(p_sky, p_hemi) per quadrature point."""
    ps = table["q_own"][Q.texel].astype(np.float64) / (2 * PI * PI * np.sqrt(Q.d[:, 0] ** 2 + Q.d[:, 2] ** 2))
    return ps, p_hemi(n, side, technique, Q.d)


def moments_under(Q, g, p):
    """Of X = g / p with the direction drawn with density p: (I = E[X], E[X^2], E[X^3], E[X^4]).  A density that vanishes where g does
    not leaves infinite moments (and I short of the integral)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return tuple(Q.integral(np.where(g > 0, g ** k / p ** (k - 1), 0.0)) for k in (1, 2, 3, 4))


def moments(Q, table, lum, n, side, technique):
    """(I, then E[X^2] of the sky technique alone, of the hemisphere technique alone and of the mixture)."""
    g = integrand(Q, lum, n, side)
    ps, ph = densities(Q, table, n, side, technique)
    return (Q.integral(g), moments_under(Q, g, ps)[1], moments_under(Q, g, ph)[1], moments_under(Q, g, 0.5 * ps + 0.5 * ph)[1])


def relvar_and_its_error(mom, count):
    """Of `count` independent samples with the moments `mom` = (I, E2, E3, E4): the relative variance E2 / I^2 - 1, and the standard
    error of its estimate m2 / m1^2 - 1 from the sample moments (delta method: the fourth moment carries it)."""
    I, e2, e3, e4 = mom
    var_m1, var_m2, cov = (e2 - I * I) / count, (e4 - e2 * e2) / count, (e3 - I * e2) / count
    var_r = var_m2 / I ** 4 + 4 * e2 * e2 * var_m1 / I ** 6 - 4 * e2 * cov / I ** 5
    return e2 / (I * I) - 1, math.sqrt(max(var_r, 0.0))


# ------------------------------------------------------------------------------------------------------------ the sample's arm --

def env_term(S, rng, n, n32, side, trace):
    """The five draws at a vertex: (direction or None where no ray is traced, m).  Tags: mix-sky, mix-hemi, mix-noenv; mix-ambiguous
    where a hemisphere direction's texel set has more than one member (spec_scenes.compare_arm leaves the sample out: sample() below)."""
    u = [F32(next(rng)) for _ in range(5)]
    hh, ww = S.env.shape[:2]
    r = draw(S.env_table, ww, hh, n32[None], [F32(side)], S.bounce, *[[x] for x in u])
    if bool(r["hemi"][0]):
        trace.append("mix-hemi")
        if int(set_size(r["u"], r["v"], ww, hh, r["du"], r["dv"])[0]) > 1:
            trace.append("mix-ambiguous")
        if bool(r["fallback"][0]):
            trace.append("cos-fallback")
    elif bool(r["wrong"][0]):
        trace.append("mix-noenv")
        return None, 0.0
    else:
        trace.append("mix-sky")
    return r["d"][0], float(r["m"][0])


def indirect_dir(S, rng, n, n32, side, flip, trace):
    """The indirect ray of the render's bounce sampling: (direction, what stands where the reference has |dot(n, w)|)."""
    if S.bounce == COSINE:
        w, fb = bounce_spec.bounce_dir(rng, n32, side, flip, trace, "cos-indirect")
        return w, (lambda v: bounce_spec.weight(n, v, fb))
    w = jade_spec.sphere_dir(rng)
    return (-w if flip(w) else w), (lambda v: abs(v @ n))


def diffuse_like(S, rng, obj, src, out, n, f, fr, scale, trace, sss=False):
    """jade_spec.diffuse_like / bounce_spec.diffuse_like / mis_spec.diffuse_like with the environment draw replaced."""
    n32 = S.norm32[obj]
    side = out @ n
    flip = lambda w: (w @ n) * side < 0
    L = (mis_spec.direct_diffuse if S.direct_mis else jade_spec.direct_diffuse)(S, rng, obj, src, n, side, f, trace)
    w, m = env_term(S, rng, n, n32, F32(side), trace)
    if w is not None:
        h, _ = S.hit(src, w, obj)
        if h < 0:
            L = L + S.sky(w) * f * abs(n @ w) * 2 * PI * m
    if not next(rng) < RR:
        return L * scale, None
    w, wt = indirect_dir(S, rng, n, n32, side, flip, trace)
    h, hp = S.hit(src, w, obj)
    if S.direct_mis and h >= 0:
        L = L + mis_spec.bounce_term(S, obj, src, f, h, hp, sss, trace)
    L = L * scale
    if h >= 0 and not jade_spec.emissive_ge(S, h):
        w = -w
        return L, (L, fr * wt(w) / RR * scale, h, hp, w)
    return L, None


def bssrdf(S, rng, obj, src, out, n, k, trace):
    """jade_spec.bssrdf / bounce_spec.bssrdf with the environment draw replaced (the exit search, the profile and the emitters are
    restated word for word, as bounce_spec restates them)."""
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
    m_ = int(S.mapping[mid])
    rx, ry = next(rng), next(rng)
    Q = S.point(m_, rx, ry)
    inner = Q - src
    r = math.sqrt(inner @ inner)
    d = S.rate[m_]
    Rd = (np.exp(-r / d) + np.exp(-r / 3.0 / d)) / (d * (8 * PI * r))
    eta = S.eta[m_]
    R0 = ((eta - 1) / (eta + 1)) ** 2
    Rd = Rd * (R0 + (1 - R0) * (1 - abs(n @ out)) ** 5)
    nm, nm32 = S.norm[m_], S.norm32[m_]
    Aobj = S.prefix[S.segs[S.obj[m_]][1]]
    if abs(inner @ nm) < 1e-5 * r * math.sqrt(nm @ nm):
        trace.append("bssrdf-coplanar")

    def Fo(v):
        return R0 - (1 - R0) * (1 - abs(v @ nm)) ** 5

    L = jade_spec.direct_bssrdf(S, rng, Q, m_, nm, Rd, Fo, Aobj, trace)
    inn = inner @ nm
    w, m = env_term(S, rng, nm, nm32, F32(inn), trace)
    if w is not None:
        h, _ = S.hit(Q, w, m_)
        if h < 0:
            L = L + S.sky(w) * Fo(w) * Rd * abs(nm @ w) * 2 * m
    L = L * (k / (1 - SSS))
    w, wt = indirect_dir(S, rng, nm, nm32, -inn, lambda v: (v @ nm) * inn > 0, trace)   # drawn BEFORE the roulette draw; the opposite hemisphere
    if not next(rng) < RR:
        return L, None
    h, hp = S.hit(Q, w, m_)
    if h >= 0 and not jade_spec.emissive_ge(S, h):
        w = -w
        return L, (L, Rd * Fo(w) * wt(w) * Aobj * 2 / RR * (k / (1 - SSS)), h, hp, w)
    return L, None


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
                    L, nxt = diffuse_like(S, rng, obj, src, out, n, fa, fr, k / SSS, trace, sss=True)
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


class Arm:
    """A spec for spec_scenes.compare_arm under JADE_ENV_MIXTURE with the given bounce and direct sampling: Scene(hs, env_sampling,
    light_sampling) and sample(...).  A sample with an ambiguous texel is tagged bssrdf-coplanar too, the one tag compare_arm leaves
    out by."""

    def __init__(self, bounce=UNIFORM, direct_mis=False):
        arm = self

        class Scene(mis_spec.Scene):
            def __init__(self, hs, env_sampling=2, light_sampling=0):
                super().__init__(hs, env_sampling, light_sampling)
                self.bounce, self.direct_mis = arm.bounce, arm.direct_mis

        self.bounce, self.direct_mis, self.Scene = bounce, direct_mis, Scene

    @staticmethod
    def sample(S, x, y, width, height, eye, cam, frame, trace=None):
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
        L = S.emis[h] + path_tracing(S, rng, h, hp, -d, trace)
        if "mix-ambiguous" in trace and "bssrdf-coplanar" not in trace:
            trace.append("bssrdf-coplanar")
        return L


# ------------------------------------------------------------------------------------------------------------- the device's side --

MIX_ROW = 10
INFO_TEXEL, INFO_WRONG, INFO_HEMI, INFO_OWN = 0x00ffffff, 1 << 29, 1 << 30, 1 << 31


def rows_of(u5, n, side, technique):
    """float32 [k, MIX_ROW]: (u0..u4, n[3], side, technique)."""
    u5 = np.asarray(u5, F32).reshape(-1, 5)
    k = len(u5)
    n = np.broadcast_to(np.asarray(n, F32).reshape(-1, 3), (k, 3))
    side = np.broadcast_to(np.asarray(side, F32).reshape(-1), (k,))
    return np.ascontiguousarray(np.concatenate([u5, n, side[:, None], np.full((k, 1), technique, F32)], 1), F32)


def unpack(info):
    info = np.asarray(info, np.uint32)
    return dict(texel=(info & np.uint32(INFO_TEXEL)).astype(np.int64), wrong=(info & np.uint32(INFO_WRONG)) != 0,
                hemi=(info & np.uint32(INFO_HEMI)) != 0, own=(info & np.uint32(INFO_OWN)) != 0)


def sample_device(scene, rows):
    """jade_debug_env_mix_sample on rows [k, MIX_ROW]: (direction float32 [k, 3], m float32 [k], unpack(info))."""
    import ctypes as C
    fn = scene.backend.lib.jade_debug_env_mix_sample
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    rows = np.ascontiguousarray(rows, F32)
    d = np.full((len(rows), 3), np.nan, F32)
    m = np.full(len(rows), np.nan, F32)
    info = np.zeros(len(rows), np.uint32)
    scene.backend.check(fn(scene._h, len(rows), rows.ctypes.data, d.ctypes.data, m.ctypes.data, info.ctypes.data))
    return d, m, unpack(info)


def sample_device_rng(scene, rows5, states):
    """jade_debug_env_mix_sample_rng on rows [k, 5] = (n[3], side, technique) and uint32 states [k]: (state after, direction, m, info)."""
    import ctypes as C
    fn = scene.backend.lib.jade_debug_env_mix_sample_rng
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
    rows5 = np.ascontiguousarray(rows5, F32)
    s = np.ascontiguousarray(states, np.uint32)
    after = np.zeros_like(s)
    d = np.full((len(s), 3), np.nan, F32)
    m = np.full(len(s), np.nan, F32)
    info = np.zeros(len(s), np.uint32)
    scene.backend.check(fn(scene._h, len(s), rows5.ctypes.data, s.ctypes.data, after.ctypes.data, d.ctypes.data, m.ctypes.data, info.ctypes.data))
    return after, d, m, unpack(info)


def texel_device(scene, dirs):
    """jade_debug_env_texel_of on float32 dirs [k, 3]: int64 [k]."""
    import ctypes as C
    fn = scene.backend.lib.jade_debug_env_texel_of
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    dirs = np.ascontiguousarray(dirs, F32)
    out = np.full(len(dirs), 0xffffffff, np.uint32)
    scene.backend.check(fn(scene._h, len(dirs), dirs.ctypes.data, out.ctypes.data))
    return out.astype(np.int64)


def shade_mode_env(lib, combo):
    """jade_debug_shade_mode_env_host on (env_sampling, lens, shutter, light, bounce, direct): (code, mode bits or None)."""
    import ctypes as C
    fn = lib.jade_debug_shade_mode_env_host
    fn.restype, fn.argtypes = C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_uint32)]
    mode = C.c_uint32(0xdeadbeef)
    rc = fn(*combo, C.byref(mode))
    return rc, (mode.value if rc == 0 else None)
