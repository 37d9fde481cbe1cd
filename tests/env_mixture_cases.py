"""What the tests of JADE_ENV_MIXTURE share (tests/test_env_mixture_cpu.py without a GPU, tests/test_gpu_env_mixture.py on the device): the
normals and the row lists of the draw's comparison, the sample-for-sample cases with their `need` tables, and the two sky-lit scenes."""
import numpy as np

import env_importance_spec as EI
import env_mixture_spec as spec
import spec_scenes as SP
import jaderaytracerendering_amd as J
from jaderaytracerendering_amd import _abi, backend as B, host as H

F32 = np.float32
UNI, COS = _abi.BOUNCE_UNIFORM, _abi.BOUNCE_COSINE
MIX = _abi.ENV_MIXTURE
ONE = F32(1.0)
HALF = F32(0.5)
U0_EDGES = np.array([0.0, np.nextafter(HALF, F32(0)), HALF, np.nextafter(HALF, F32(1)), 1.0], F32)
MAPS = [(w, h, kind) for (w, h) in EI.MAP_SIZES for kind in EI.KINDS]


def normals():
    """fp32 [k, 3]: the axes both ways, random unit normals, those x 2.5, and the normals that give the cosine draw no axis (zero, NaN,
    inf)."""
    rng = np.random.default_rng(316)
    v = rng.normal(size=(6, 3))
    unit = (v / np.sqrt((v * v).sum(-1))[:, None]).astype(F32)
    nan, inf = F32(np.nan), F32(np.inf)
    return np.concatenate([np.eye(3, dtype=F32), -np.eye(3, dtype=F32), unit, unit * F32(2.5), np.zeros((1, 3), F32),
                           np.array([[nan, 0.5, 0.5], [0.5, inf, 0.5]], F32)])


def rows(table, w, h, technique):
    """float32 [k, MIX_ROW] = (u0..u4, n[3], side, technique): 20 000 random rows, then the edge rows -
      * u0 at 0, pred(0.5), 0.5, succ(0.5) and 1.0f with random partners, under every normal and both sides;
      * sky rows (u0 = 0): every edge row of tests/test_gpu_env_importance.py's uniform_rows, none left out or sampled (31 N + about 3 N
        rows) - every slot's middle, u1 at 0, 1.0f and every k / N with both fp32 neighbours, u2 at 0, 1.0f, accept and an ulp to either
        side, u3 and u4 at 0, 1.0f and 1 - 2^-24 crossed for the own and the alias texel of every slot and once more with a random
        partner - with a normal from the list in turn and the side alternating;
      * hemisphere rows (u0 = 1) under the normals +-y with both sides: the cosine draw's poles (u1 = 0), the uniform draw's ends
        (u1 = 0, 1.0f), the seam (u2 = 0.5 and an ulp to either side: z = +-0 and x < 0; with u1 = 0.5 for the uniform draw), and
        directions within 2 ulp of u1 / u2 of a texel's border (_border_uniforms: a few, so that at most 1 % of a map's hemisphere
        rows are ambiguous - tests/test_env_mixture_cpu.py holds the lists to that)."""
    n = w * h
    rng = np.random.default_rng(29 * w + h + 7 * technique)
    N = normals()
    out = []

    def add(u5, nrm, side):
        out.append(spec.rows_of(u5, nrm, side, technique))

    k = 20000
    u = (rng.integers(0, 2 ** 32, size=(k, 5), dtype=np.uint64).astype(F32) * F32(2.0 ** -32)).astype(F32)
    add(u, N[rng.integers(0, len(N), size=k)], np.where(rng.random(k) < 0.5, F32(-1), F32(1)))
    for u0 in U0_EDGES:
        for side in (F32(1), F32(-1)):
            u = rng.random((len(N), 5), dtype=F32)
            u[:, 0] = u0
            add(u, N, side)
    # the sky rows: tests/test_gpu_env_importance.py's uniform_rows, block for block (its 30 000 random rows are the random rows above)
    mid = ((np.arange(n) + 0.5) / n).astype(F32)          # one u1 per slot
    edge = np.array([0.0, ONE, np.nextafter(ONE, F32(0))], F32)
    sky = [np.column_stack([mid, rng.random((n, 3), dtype=F32)])]
    # u1 at 0, at 1.0f and at k / N with both neighbours: the edges of the fp32 slot product
    kk = (np.arange(n + 1) / n).astype(F32)
    u1 = np.unique(np.clip(np.concatenate([kk, np.nextafter(kk, F32(-1)), np.nextafter(kk, F32(2)), [F32(0), ONE]]), 0, 1).astype(F32))
    sky.append(np.column_stack([u1, rng.random((len(u1), 3), dtype=F32)]))
    for u2 in (F32(0), ONE):  # ... and the two ends once more with the own and the alias texel
        sky.append(np.column_stack([np.array([0, ONE], F32), np.full(2, u2), rng.random((2, 2), dtype=F32)]))
    # u2 at accept and one ulp to either side, for every slot
    acc = table["accept"][EI.slot_of(mid, n)]
    for u2 in (acc, np.nextafter(acc, F32(-1)), np.nextafter(acc, F32(2))):
        sky.append(np.column_stack([mid, np.clip(u2, 0, 1).astype(F32), rng.random((n, 2), dtype=F32)]))
    # u3, u4 at 0, 1.0f and 1 - 2^-24 for the own and the alias texel of every slot: the seam column and both pole rows among them
    for u2 in (F32(0), ONE):
        for u3 in edge:
            for u4 in edge:
                sky.append(np.column_stack([mid, np.full(n, u2), np.full(n, u3), np.full(n, u4)]))
    # ... and crossed with a random partner
    for col in (2, 3):
        for val in edge:
            r = rng.random((n, 4), dtype=F32)
            r[:, 0], r[:, col] = mid, val
            sky.append(r)
    sky = np.concatenate(sky).astype(F32)
    idx = np.arange(len(sky)) % len(N)
    add(np.column_stack([np.zeros(len(sky), F32), sky]), N[idx], np.where((np.arange(len(sky)) // len(N)) % 2 == 0, F32(1), F32(-1)))
    # the hemisphere rows: poles and seam under the normals +-y (cosine about +-y: d = (r cs, +-cz, -+r sn); uniform: d = (sin cs, sin sn, c))
    ey = np.eye(3, dtype=F32)[1]
    u12 = np.array([(a, b) for a in (0.0, HALF, ONE) for b in (0.0, HALF, np.nextafter(HALF, F32(0)), np.nextafter(HALF, F32(1)))], F32)
    for nrm in (ey, -ey):
        for side in (F32(1), F32(-1)):
            u = rng.random((len(u12), 5), dtype=F32)
            u[:, 0], u[:, 1:3] = ONE, u12
            add(u, nrm, side)
    # ... and within 2 ulp of a texel's border: the last uniform on one side of it and the first on the other, found by bisection over the
    # fp32 values of u1 (col = 1) or u2 (col = 2) with the statement's own texel, and the neighbour of each
    for col in (1, 2):
        b = _border_uniforms(w, h, technique, ey, col, 6, rng)
        if len(b):
            u = rng.random((len(b), 5), dtype=F32)
            u[:, 0], u[:, 1:3] = ONE, b
            add(u, ey, F32(1))
    return np.ascontiguousarray(np.concatenate(out), F32)


def _border_uniforms(w, h, technique, nrm, col, count, rng):
    """(u1, u2) pairs, fp32 [<= 4 count, 2], whose hemisphere direction about nrm (side +1) lies within 2 ulp of the moved uniform of a
    border between two texels: rows of the map are crossed by moving u1 or u2, whichever `col` names."""
    k = 2048
    lo = (rng.random((k, 2)) * 0.8 + 0.1).astype(F32)
    hi = lo.copy()
    hi[:, col - 1] += F32(0.03)

    def texel(u12):
        d, _, _, _ = spec.hemisphere(np.tile(nrm, (len(u12), 1)), np.ones(len(u12), F32), technique, u12[:, 0], u12[:, 1])
        return spec.texel_of(d, w, h)[0]

    keep = np.flatnonzero(texel(lo) != texel(hi))[:count]
    if len(keep) == 0:
        return np.zeros((0, 2), F32)
    lo, hi = lo[keep], hi[keep]
    t_lo = texel(lo)
    a, b = lo[:, col - 1].copy().view(np.int32), hi[:, col - 1].copy().view(np.int32)
    while (b - a > 1).any():
        mid = a + (b - a) // 2
        trial = lo.copy()
        trial[:, col - 1] = mid.view(F32)
        same = texel(trial) == t_lo
        a, b = np.where(same, mid, a).astype(np.int32), np.where(same, b, mid).astype(np.int32)
    out = []
    for bits in (a - 1, a, b, b + 1):
        r = lo.copy()
        r[:, col - 1] = bits.astype(np.int32).view(F32)
        out.append(r)
    return np.concatenate(out)


def spec_draw(table, w, h, r, technique, texel=None):
    return spec.draw(table, w, h, r[:, 5:8], r[:, 8], technique, r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], texel=texel)


# ------------------------------------------------------------------------------------------------------ sample for sample --
MAX_LEFT_OUT = 0.05
LIGHTS_ONE = _abi.LIGHTS_ONE
# 12 x 12 frames at 1 spp under the 8 x 4 map with one bright texel (spec_scenes.sky_map).  `need`: half of what the arm alone counts for
# every tag on these samples (the comment above each case; tests/test_env_mixture_cpu.py holds the tables to these counts).
ARMS = {
    # the arm alone: 432 samples, 11 left out (2.5 %): 16 bssrdf, 224 diffuse, 62 mirror, 131 mix-hemi, 44 mix-noenv, 100 mix-sky, 152 sky,
    # 32 sss
    "jade_cube-uniform": dict(kind="jade_cube", bounce=UNI, frames=(0, 1, 2),
        need={"bssrdf": 8, "diffuse": 112, "mirror": 31, "mix-hemi": 65, "mix-noenv": 22, "mix-sky": 50, "sky": 76, "sss": 16}),
    # the arm alone: 432 samples, 13 left out (3.0 %): 20 bssrdf, 222 cos-indirect, 222 diffuse, 66 mirror, 127 mix-hemi, 50 mix-noenv, 105
    # mix-sky, 152 sky, 38 sss
    "jade_cube-cosine": dict(kind="jade_cube", bounce=COS, frames=(0, 1, 2),
        need={"bssrdf": 10, "cos-indirect": 111, "diffuse": 111, "mirror": 33, "mix-hemi": 63, "mix-noenv": 25, "mix-sky": 52, "sky": 76, "sss": 19}),
    # the arm alone: 432 samples, 0 left out (0.0 %): 239 diffuse, 117 mix-hemi, 31 mix-noenv, 91 mix-sky, 191 sky
    "open_floor-uniform": dict(kind="open_floor", bounce=UNI, frames=(0, 1, 2),
        need={"diffuse": 119, "mix-hemi": 58, "mix-noenv": 15, "mix-sky": 45, "sky": 95}),
    # the arm alone: 432 samples, 0 left out (0.0 %): 216 cos-indirect, 239 diffuse, 117 mix-hemi, 31 mix-noenv, 91 mix-sky, 191 sky
    "open_floor-cosine": dict(kind="open_floor", bounce=COS, frames=(0, 1, 2),
        need={"cos-indirect": 108, "diffuse": 119, "mix-hemi": 58, "mix-noenv": 15, "mix-sky": 45, "sky": 95}),
    # the arm alone: 576 samples, 7 left out (1.2 %): 10 bssrdf, 309 diffuse, 49 mirror, 166 mix-hemi, 78 mix-noenv, 103 mix-sky, 14
    # refract, 3 refract-open, 202 sky, 19 sss
    "patchwork-uniform": dict(kind="patchwork", bounce=UNI, frames=(0, 1, 2, 3),
        need={"bssrdf": 5, "diffuse": 154, "mirror": 24, "mix-hemi": 83, "mix-noenv": 39, "mix-sky": 51, "refract": 7, "refract-open": 1, "sky": 101, "sss": 9}),
    # the arm alone: 576 samples, 6 left out (1.0 %): 8 bssrdf, 305 cos-indirect, 309 diffuse, 52 mirror, 171 mix-hemi, 79 mix-noenv, 103
    # mix-sky, 13 refract, 2 refract-open, 202 sky, 16 sss
    "patchwork-cosine": dict(kind="patchwork", bounce=COS, frames=(0, 1, 2, 3),
        need={"bssrdf": 4, "cos-indirect": 152, "diffuse": 154, "mirror": 26, "mix-hemi": 85, "mix-noenv": 39, "mix-sky": 51, "refract": 6, "refract-open": 1, "sky": 101, "sss": 8}),
    # the arm alone: 432 samples, 11 left out (2.5 %): 16 bssrdf, 11 bssrdf-lit, 224 diffuse, 118 diffuse-lit, 87 light-alias, 142 light-
    # lit, 180 light-own, 116 light-shadowed, 12 light-side, 62 mirror, 131 mix-hemi, 44 mix-noenv, 100 mix-sky, 142 sky, 32 sss, 16 sss-lit
    "two_lamps-uniform": dict(kind="two_lamps", bounce=UNI, light_sampling=LIGHTS_ONE, frames=(0, 1, 2),
        need={"bssrdf": 8, "bssrdf-lit": 5, "diffuse": 112, "diffuse-lit": 59, "light-alias": 43, "light-lit": 71, "light-own": 90, "light-shadowed": 58, "light-side": 6, "mirror": 31, "mix-hemi": 65, "mix-noenv": 22, "mix-sky": 50, "sky": 71, "sss": 16, "sss-lit": 8}),
    # the arm alone: 432 samples, 13 left out (3.0 %): 20 bssrdf, 15 bssrdf-lit, 222 cos-indirect, 222 diffuse, 117 diffuse-lit, 88 light-
    # alias, 143 light-lit, 178 light-own, 116 light-shadowed, 18 light-side, 66 mirror, 127 mix-hemi, 50 mix-noenv, 105 mix-sky, 142 sky,
    # 38 sss, 19 sss-lit
    "two_lamps-cosine": dict(kind="two_lamps", bounce=COS, light_sampling=LIGHTS_ONE, frames=(0, 1, 2),
        need={"bssrdf": 10, "bssrdf-lit": 7, "cos-indirect": 111, "diffuse": 111, "diffuse-lit": 58, "light-alias": 44, "light-lit": 71, "light-own": 89, "light-shadowed": 58, "light-side": 9, "mirror": 33, "mix-hemi": 63, "mix-noenv": 25, "mix-sky": 52, "sky": 71, "sss": 19, "sss-lit": 9}),
    # the arm alone: 432 samples, 13 left out (3.0 %): 20 bssrdf, 15 bssrdf-lit, 222 cos-indirect, 222 diffuse, 117 diffuse-lit, 88 light-
    # alias, 143 light-lit, 178 light-own, 116 light-shadowed, 18 light-side, 66 mirror, 8 mis-bounce-lit, 3 mis-sss-bounce-lit, 130 mis-
    # weighted, 127 mix-hemi, 50 mix-noenv, 105 mix-sky, 142 sky, 38 sss, 19 sss-lit
    "two_lamps-mis": dict(kind="two_lamps", bounce=COS, mis=True, light_sampling=LIGHTS_ONE, frames=(0, 1, 2),
        need={"bssrdf": 10, "bssrdf-lit": 7, "cos-indirect": 111, "diffuse": 111, "diffuse-lit": 58, "light-alias": 44, "light-lit": 71, "light-own": 89, "light-shadowed": 58, "light-side": 9, "mirror": 33, "mis-bounce-lit": 4, "mis-sss-bounce-lit": 1, "mis-weighted": 65, "mix-hemi": 63, "mix-noenv": 25, "mix-sky": 52, "sky": 71, "sss": 19, "sss-lit": 9}),
}
MIX_TAGS = ("mix-sky", "mix-hemi", "mix-noenv")


def compare(backend, name, **kw):
    """spec_scenes.compare_arm for one case of ARMS (count_only=True: the arm alone, no backend)."""
    c = ARMS[name]
    modes = [("set_bounce_sampling", c["bounce"])] + ([("set_direct_sampling", _abi.DIRECT_MIS)] if c.get("mis") else [])
    return SP.compare_arm(spec.Arm(c["bounce"], bool(c.get("mis"))), f"mixture {name} ", modes, SP.build, backend, c["kind"], 12, c["frames"], c["need"],
                          sky=True, env_sampling=MIX, light_sampling=c.get("light_sampling", _abi.LIGHTS_ALL), max_left_out=MAX_LEFT_OUT, **kw)


# ------------------------------------------------------------------------------------------------------------- the scenes --
BALL_W, BALL_H = 48, 40


def sky_lit_ball():
    """tests/test_gpu_env_sampling.py's scene again: a diffuse ball and a diffuse slab under the procedural 64 x 32 sky (gradient + sun
    lobe), no emitter - all light is environment light.  (the host scene, the camera's config)"""
    cfg = J.SceneBuilder().config("tiny")
    b = J.SceneBuilder()
    b.add_proc("geodesic", 3, H.material(brdf=(0.6, 0.55, 0.5)), H.transform_matrix(trans=(0.1, -1.2, 1.0), scale=(1.1, 1.1, 1.1)))
    b.add_proc("box", 0, H.material(brdf=(0.5, 0.5, 0.5)), H.transform_matrix(trans=(0.0, -2.3, 1.0), scale=(9.0, 0.2, 9.0)))
    b.set_env_sky(64, 32)
    return b.build(), cfg


def ball_params(cfg, spp, env, frame=0):
    p = B.params_from_config(cfg, spp=spp)
    p.width, p.height = BALL_W, BALL_H
    p.walk, p.env_sampling, p.frame = _abi.WALK_EARLY_EXIT, env, frame
    return p


FLOOR_BRDF = (0.6, 0.5, 0.4)


def open_floor_sky():
    """A diffuse floor (normal +y, seen from above) under the procedural 64 x 32 sky and nothing else: no emitter, nothing to occlude, so a
    floor pixel's sample is its ONE environment term."""
    b = J.SceneBuilder()
    b.add_mesh(SP.quad(-0.9, 30.0), SP.QUAD_I, H.material(brdf=FLOOR_BRDF))
    b.set_env_sky(64, 32)
    return b.build()


def floor_params(spp, env, frame=0):
    eye, cam = H.camera_orbit(2.8, 50.0, 10.0)
    return B.make_params(BALL_W, BALL_H, spp, eye, cam, frame=frame, threads=2, env_sampling=env, walk=_abi.WALK_EARLY_EXIT)
