"""What the texture tests share (include/jade_bvh.h, "The surface colour, stated"): putting a table on a host scene, the scene with a
colour per triangle baked into its materials, and the six scenes of the sample-for-sample comparison with their `need` tables (compared
in tests/test_gpu_texture.py, counted by count() below on the CPU).  Nothing here opens a device."""
import math
import types

import numpy as np

import jaderaytracerendering_amd as J
import smooth_cases as SC
import spec_scenes as SP
import texture_spec
from jaderaytracerendering_amd import _abi, host as H

F32 = np.float32


def copy_scene(hs):
    out = H.HostScene({k: v.copy() for k, v in hs.a.items()}, hs.bvh_depth, vertex_normals=None if hs.vertex_normals is None else hs.vertex_normals.copy())
    out.textures = getattr(hs, "textures", None)
    return out


def planar_uv(hs, seed=11, scale=0.8):
    """float32 [n, 3, 2]: every corner's position through one random affine map - shared edges share their UVs, and with |rows| up to
    `scale` per unit of length a wrap seam (u or v an integer) crosses the triangles of any object larger than 1 / scale."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-scale, scale, (3, 2))
    off = rng.uniform(0, 1, 2)
    return (hs.vertices().astype(np.float64) @ A + off).astype(F32)


def random_image(seed=12, size=16, lo=0.2, hi=1.4):
    return np.random.default_rng(seed).uniform(lo, hi, (size, size, 3)).astype(F32)


def textured(hs, images, image_of=None, uv=None):
    """hs with hs.textures = (images, uv, image_of): Backend.scene() puts it on the handle, texture_spec.Scene reads it."""
    n = hs.n_triangles
    hs.textures = (list(images), planar_uv(hs) if uv is None else np.ascontiguousarray(uv, F32).reshape(n, 3, 2),
                   np.zeros(n, np.int32) if image_of is None else np.ascontiguousarray(image_of, np.int32))
    return hs


def baked(hs, c):
    """A copy of hs without textures whose triangles carry fl(brdf * c) and fl(refract_albedo * c); c: float32 [3] or [n, 3]."""
    out = copy_scene(hs)
    out.textures = None
    t = out.tri_f32()
    c = np.broadcast_to(np.asarray(c, F32), (hs.n_triangles, 3))
    t[:, 16:19] = t[:, 16:19] * c
    t[:, 24:27] = t[:, 24:27] * c
    return out


# ---- the floor and the mirror-and-wall scene of the closed forms and the guide tests ----
FLOOR_Y, FLOOR_S = -0.9, 12.0
WALL_Y, WALL_S = 5.0, 40.0


def corner_ray(p, x, y, rx, ry):
    """jade_spec.sample's camera ray with the two jitter draws given: (rx, ry) in {0, 1}^2 are the corners of pixel (x, y)."""
    lx = (-1 + 2.0 / p.width * (x + rx - 0.5)) * (p.width / p.height)
    ly = -1 + 2.0 / p.height * (y + ry - 0.5)
    M = np.asarray(list(p.camera), np.float64).reshape(4, 4)
    v = np.array([lx, ly, -1.5, 0.0])
    d = np.array([sum(M[c][r] * v[c] for c in range(4)) for r in range(3)])
    return np.asarray(list(p.eye), np.float64), d / math.sqrt(d @ d)


def mirror_and_wall(wall_image, floor_image):
    """A mirror floor (brdf 0.9 0.8 0.7) and a diffuse wall (brdf 0.8 0.7 0.6) lying overhead at y = 5, facing down, u = 0.5 + x / 96: the
    camera looks down at the floor - no camera ray meets the wall - and sees the wall in it."""
    b = J.SceneBuilder()
    try:
        b.add_mesh(SP.quad(FLOOR_Y, FLOOR_S), SP.QUAD_I, H.material(brdf=(0.9, 0.8, 0.7), reflex_mode=_abi.MIRROR))
        b.add_mesh(SP.quad(WALL_Y, WALL_S, flip=True), SP.QUAD_I, H.material(brdf=(0.8, 0.7, 0.6)))
        b.set_env_constant(0.5, 0.6, 0.8)
        hs = b.build()
    finally:
        b.close()
    v = hs.vertices().astype(np.float64)
    uv = (0.5 + v[:, :, [0, 2]] / (2.4 * WALL_S)).astype(F32)
    is_wall = np.abs(hs.vertices()[:, :, 1] - WALL_Y).max(1) < 1e-6
    assert is_wall.sum() == 2
    return textured(hs, [wall_image, floor_image], image_of=np.where(is_wall, 0, 1), uv=uv), is_wall


# ---- the six scenes, each with a random 16 x 16 image on every triangle through planar_uv ----
SSS_DIFFUSE = dict(SP.JADE, reflex_mode=_abi.DIFFUSE)
MIRROR_FLOOR = dict(SP.FLOOR, reflex_mode=_abi.MIRROR)


def _over(floor, add):
    b = J.SceneBuilder()
    add(b)
    b.add_mesh(SP.quad(1.5, 0.5, flip=True), SP.QUAD_I, H.material(**SP.LIGHT))
    b.add_mesh(SP.quad(-0.9, 3.0), SP.QUAD_I, H.material(**floor))
    b.set_env_constant(0.5, 0.6, 0.8)
    return b.build()


def build(kind, sky=False):
    rot = H.transform_matrix(rot_deg=(20, 30, 0))
    if kind == "diffuse":
        hs = _over(SP.FLOOR, lambda b: b.add_mesh(SP.CUBE_V, SP.CUBE_I, H.material(**SC.DIFFUSE), rot))
    elif kind == "sss_diffuse":
        hs = _over(SP.FLOOR, lambda b: b.add_mesh(SP.CUBE_V, SP.CUBE_I, H.material(**SSS_DIFFUSE), rot))
    elif kind == "jade":
        hs = SP.build("jade_cube")
    elif kind == "mirror_floor":       # the diffuse cube seen in the floor, whose own image tints the reflection
        hs = _over(MIRROR_FLOOR, lambda b: b.add_mesh(SP.CUBE_V, SP.CUBE_I, H.material(**SC.DIFFUSE), rot))
    elif kind == "under_glass":        # the floor seen through the glass cube
        hs = SP.build("glass_cube")
    elif kind == "smooth_jade":        # vertex normals as well
        hs = SC.ball(SP.JADE)
        assert hs.vertex_normals is not None
    else:
        raise ValueError(kind)
    return textured(hs, [random_image()])


def arm(cosine=False):
    def sample(S, x, y, width, height, eye, cam, frame, trace=None):
        trace = trace if trace is not None else []
        out = texture_spec.sample(S, x, y, width, height, eye, cam, frame, trace)
        if "smooth-undecided" in trace and "bssrdf-coplanar" not in trace:      # (tests/smooth_cases.py: compare_arm knows the one tag)
            trace.append("bssrdf-coplanar")
        return out

    return types.SimpleNamespace(Scene=lambda hs, env_sampling=0, light_sampling=0: texture_spec.Scene(hs, env_sampling, light_sampling, cosine), sample=sample)


SIZE, FRAMES = 12, tuple(range(8))
# `need`: half of what the arm alone counts on these 1152 samples (count(); a sample counts once per tag)
CASES = {
    # the arm alone, 0 left out: 732 diffuse, 414 sky, 732 smooth-flat, 732 textured
    "diffuse": dict(need={"diffuse": 366, "sky": 207, "smooth-flat": 366, "textured": 366}),
    # the arm alone, 33 left out: 37 bssrdf, 645 diffuse, 414 sky, 699 smooth-flat, 89 sss, 699 textured
    "sss_diffuse": dict(need={"bssrdf": 18, "diffuse": 322, "sky": 207, "smooth-flat": 349, "sss": 44, "textured": 349}),
    # the arm alone, 25 left out: 47 bssrdf, 576 diffuse, 168 mirror, 414 sky, 707 smooth-flat, 106 sss, 707 textured
    "jade": dict(need={"bssrdf": 23, "diffuse": 288, "mirror": 84, "sky": 207, "smooth-flat": 353, "sss": 53, "textured": 353}),
    # the arm alone, 0 left out: 317 diffuse, 570 mirror, 414 sky, 732 smooth-flat, 732 textured
    "mirror_floor": dict(need={"diffuse": 158, "mirror": 285, "sky": 207, "smooth-flat": 366, "textured": 366}),
    # the arm alone, 0 left out: 625 diffuse, 148 mirror, 145 refract, 14 refract-open, 414 sky, 732 smooth-flat, 732 textured
    "under_glass": dict(need={"diffuse": 312, "mirror": 74, "refract": 72, "refract-open": 7, "sky": 207, "smooth-flat": 366, "textured": 366}),
    # the arm alone, 2 left out: 61 bssrdf, 567 diffuse, 158 mirror, 431 sky, 241 smooth, 42 smooth-culled, 567 smooth-flat, 8 smooth-redirect, 10 smooth-side, 110 sss, 713 textured
    "smooth_jade": dict(need={"bssrdf": 30, "diffuse": 283, "mirror": 79, "sky": 215, "smooth": 120, "smooth-culled": 21, "smooth-flat": 283, "smooth-redirect": 4, "smooth-side": 5, "sss": 55, "textured": 356}),
}
LEFT_OUT_CAP = 0.07   # bssrdf-coplanar and smooth-undecided together (tests/smooth_cases.py: 5 % + 2 %); the texture adds none


def run(name, backend=None, out=None):
    c = CASES[name]
    return SP.compare_arm(arm(), "textured ", [], build, backend, name, SIZE, FRAMES, c["need"] if backend is not None else {}, out=out,
                          count_only=backend is None, max_left_out=LEFT_OUT_CAP)


def count():
    """What the arm alone counts per case: python tests/texture_cases.py prints the tables the `need` entries above are half of."""
    for name in CASES:
        seen, _, n, skipped = run(name)
        print(name, n, skipped, dict(sorted(seen.items())))


if __name__ == "__main__":
    count()
