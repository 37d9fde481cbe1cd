"""Three crafted scenes for the guide pass (include/jade_bvh.h, "Guides of pixel (x, y)"), which reach the vertices that tinyjade and C1
never do (tests/test_denoise_cpu.py counts them, tests/test_gpu_denoise_exact.py holds the device to them).

  mirrors   two facing mirrors, the camera between them: every chain passes JADE_MAX_FULL_REFLEX_TIME = 32 mirror vertices and ends at
            the 33rd by the limit - a = brdf^33, z = the summed distances
  tinted    a wall of three mirrors whose emission is 2e-4 in red only, in green only and in blue only, a diffuse wall behind the camera:
            the render's mirror test reads emissive[0], [1] and [0] again, so red and green end the chain and blue does not
  behind    two quads of opposite winding beside open sky: one of them is seen from behind (its normal comes back negated), a miss
            gives a = t = 1, n = 0, z = 0

The camera is the identity matrix at the origin: it looks down -z.  Frames are 16 x 12, which is no multiple of the tile."""
import math

import numpy as np

from jaderaytracerendering_amd import _abi, backend as B, host as H

import jade_spec

WIDTH, HEIGHT, FRAME = 16, 12, 3
SCENES = ("mirrors", "tinted", "behind")
LIMIT = 32  # JADE_MAX_FULL_REFLEX_TIME
QUAD_I = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
# at least this many of the 192 pixels must, by the spec alone (counted on the CPU):
NEED = {"mirrors": {"limit": 180}, "tinted": {"red": 40, "green": 40, "blue passed": 40}, "behind": {"back face": 40, "front face": 40, "miss": 40}}


def _quad(x0, x1, y0, y1, z, flip=False):
    v = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float32)
    return v[::-1].copy() if flip else v


def _mirror(brdf, emissive=(0, 0, 0)):
    return H.material(brdf=brdf, emissive=emissive, reflex_mode=_abi.MIRROR)


def _build(name):
    b = H.SceneBuilder()
    try:
        if name == "mirrors":
            b.add_mesh(_quad(-200, 200, -200, 200, -2.0), QUAD_I, _mirror((0.9, 0.8, 0.95)))
            b.add_mesh(_quad(-200, 200, -200, 200, 2.0, flip=True), QUAD_I, _mirror((0.9, 0.8, 0.95)))
        elif name == "tinted":
            b.add_mesh(_quad(-3.0, -0.6, -3, 3, -2.0), QUAD_I, _mirror((0.9, 0.5, 0.5), (2e-4, 0, 0)))
            b.add_mesh(_quad(-0.6, 0.6, -3, 3, -2.0), QUAD_I, _mirror((0.5, 0.9, 0.5), (0, 2e-4, 0)))
            b.add_mesh(_quad(0.6, 3.0, -3, 3, -2.0), QUAD_I, _mirror((0.5, 0.5, 0.9), (0, 0, 2e-4)))
            b.add_mesh(_quad(-20, 20, -20, 20, 2.0, flip=True), QUAD_I, H.material(brdf=(0.6, 0.7, 0.8)))
        elif name == "behind":
            b.add_mesh(_quad(-3.0, -0.6, -3, 3, -2.0), QUAD_I, H.material(brdf=(0.6, 0.5, 0.4)))
            b.add_mesh(_quad(-0.6, 0.6, -3, 3, -2.5, flip=True), QUAD_I, H.material(brdf=(0.3, 0.5, 0.7)))
        else:
            raise ValueError(name)
        b.set_env_sky(16, 8)
        return b.build()
    finally:
        b.close()


_scenes = {}


def scene(name):
    """Built once; callers do not edit what they get."""
    if name not in _scenes:
        _scenes[name] = _build(name)
    return _scenes[name]


def params(spp=4, **kw):
    return B.make_params(WIDTH, HEIGHT, spp, (0.0, 0.0, 0.0), np.eye(4, dtype=np.float32).ravel(), frame=FRAME, **kw)


def camera_ray(x, y, p, frame):
    """The camera ray of sample `frame - p.frame` of pixel (x, y) in float64, as spec_guide below makes it."""
    rng = jade_spec.wang_stream(x, y, frame)
    lx = (-1 + 2.0 / p.width * (x + next(rng) - 0.5)) * (p.width / p.height)
    ly = -1 + 2.0 / p.height * (y + next(rng) - 0.5)
    M = np.asarray(list(p.camera), np.float64).reshape(4, 4)
    v = np.array([lx, ly, -1.5, 0.0])
    d = np.array([sum(M[c][r] * v[c] for c in range(4)) for r in range(3)])
    return np.asarray(list(p.eye), np.float64), d / math.sqrt(d @ d)


def classify(S, x, y, p, frame):
    """What the guide sample of pixel (x, y) meets, by the header's text: the set of the names NEED counts."""
    o, d = camera_ray(x, y, p, frame)
    skip, seen = -1, set()
    for k in range(LIMIT + 1):
        h, hp = S.hit(o, d, skip)
        if h < 0:
            return seen | {"miss"}
        e = S.emis[h]
        mirror = S.reflex[h] == _abi.MIRROR
        ends = e[0] > 1.5e-4 or e[1] > 1.5e-4  # (the render's test reads emissive[0] twice and never [2])
        if mirror and not ends and k < LIMIT:
            if e[2] > 1.5e-4:
                seen.add("blue passed")
            n = S.norm[h]
            d = n * (2 * (-d @ n)) + d
            o, skip = hp, h
            continue
        if mirror and ends:
            seen.add("red" if e[0] > 1.5e-4 else "green")
        elif mirror:
            seen.add("limit")
        seen.add("back face" if S.norm[h] @ d > 0 else "front face")
        return seen
    raise AssertionError("unreachable")


def counts(S, p):
    out = {}
    for y in range(p.height):
        for x in range(p.width):
            for name in classify(S, x, y, p, p.frame):
                out[name] = out.get(name, 0) + 1
    return out


# ---- the float64 statement of the guide pass, on any scene (tests/test_gpu_denoise.py holds the device's guides to it) ----

def spec_guide(S, x, y, p, frame):
    """jade_bvh.h's guide sample in float64: (albedo, normal, depth)."""
    rng = jade_spec.wang_stream(x, y, frame)
    lx = (-1 + 2.0 / p.width * (x + next(rng) - 0.5)) * (p.width / p.height)
    ly = -1 + 2.0 / p.height * (y + next(rng) - 0.5)
    M = np.asarray(list(p.camera), np.float64).reshape(4, 4)
    v = np.array([lx, ly, -1.5, 0.0])
    d = np.array([sum(M[c][r] * v[c] for c in range(4)) for r in range(3)])
    d = d / math.sqrt(d @ d)
    o = np.asarray(list(p.eye), np.float64)
    t, z, skip = np.ones(3), 0.0, -1
    for k in range(33):  # JADE_MAX_FULL_REFLEX_TIME mirror vertices, then the final one
        h, hp = S.hit(o, d, skip)
        if h < 0:
            return t, np.zeros(3), 0.0
        dist = (hp - o) @ (d / math.sqrt(d @ d))
        e = S.emis[h]
        if S.reflex[h] == _abi.MIRROR and not (e[0] > 1.5e-4 or e[1] > 1.5e-4 or e[0] > 1.5e-4) and k < 32:
            t = t * S.brdf[h]
            z += dist
            out = -d
            n = S.norm[h]
            d = n * (2 * (out @ n)) - out
            o, skip = hp, h
            continue
        z += dist
        n = S.norm[h]
        return t * S.brdf[h], (-n if n @ d > 0 else n), z
    raise AssertionError("mirror chain too long")


class Geometry:
    """What jade_spec.Scene.hit reads of a scene (the geometry alone: the guides never look at the environment)."""
    hit = jade_spec.Scene.hit

    def __init__(self, hs):
        t = hs.a["triangles"]
        f, i = t.view(np.float32).astype(np.float64), t.view(np.int32)
        self.p1, self.p2, self.p3 = f[:, 1:4], f[:, 4:7], f[:, 7:10]
        self.norm, self.emis, self.brdf = f[:, 10:13], f[:, 13:16], f[:, 16:19]
        self.reflex = i[:, 19]
        self.n = len(t)
