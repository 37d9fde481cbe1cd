"""What the normal-map tests share (include/jade_bvh.h, "The mapped normal, stated"): putting a map table on a host scene, and the seven
scenes of the sample-for-sample comparison with their `need` tables (compared in tests/test_gpu_normal_map.py, counted by count() below on
the CPU and held to it by tests/test_normal_map_spec_cpu.py).  Nothing here opens a device."""
import types

import numpy as np

import normal_map_spec
import spec_scenes as SP
import texture_cases as TC

F32 = np.float32


def mapped(hs, images, image_of=None, uv=None, strength=1.0):
    """hs with hs.normal_maps = (images, uv, image_of, strength): Backend.scene() puts it on the handle, normal_map_spec.Scene reads it."""
    n = hs.n_triangles
    hs.normal_maps = (list(images), TC.planar_uv(hs, seed=21) if uv is None else np.ascontiguousarray(uv, F32).reshape(n, 3, 2),
                      np.zeros(n, np.int32) if image_of is None else np.ascontiguousarray(image_of, np.int32), float(strength))
    return hs


def random_map(seed=22, size=16, tilt=0.35, zero_block=True):
    """size x size tangent-space vectors (x, y, 1) with x, y uniform in [-tilt, tilt]: a moderate tilt - up to ~26 degrees off the base at
    tilt = 0.35 - so that the bent normal is on the wrong side of a grazing ray now and then and a drawn direction is culled against g, and
    never so small that a tilt is within its bound of zero - except in one block of 6 x 6 texels (0, 0, 1), whose inside has no tilt at all."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-tilt, tilt, (size, size, 2))
    xy = np.where(np.abs(xy) < 0.02, 0.02, xy)
    if zero_block:
        xy[2:8, 5:11] = 0.0
    return np.concatenate([xy, np.ones((size, size, 1))], -1).astype(F32)


# the cube's own image in under_glass: "low" is the case's; "high" is what the other triangles carry, kept for the CPU test of the claim above
GLASS_MAPS = {"low": lambda: random_map(seed=23, size=2, tilt=0.2, zero_block=False), "high": lambda: random_map()}


def build(kind, sky=False, glass_map="low"):
    """texture_cases' six scenes under a random 16 x 16 map on every triangle (the map's own planar UVs), the albedo table kept on
    `all_three` - vertex normals, albedo and map together - and dropped on the others.
    under_glass gives the glass cube itself (object 0) a second image, a 2 x 2 random map of tilt 0.2: the refraction loop's mapped normal
    - at the entry, at every inner reflection, at the exit - is then held sample for sample, on a map the statement is well-conditioned
    under.  Under the 16 x 16 map a glass body is a chaotic billiard for the rays reflected inside it - every face bends its normal at 16
    texels per unit - and the float64 statement itself does not say what such a path returns to 1e-4: GLASS_MAPS and
    tests/test_normal_map_spec_cpu.py, which moves the strength by 2e-7 of its value under both maps and counts the samples that move."""
    if kind == "all_three":
        hs = TC.build("smooth_jade", sky)
    else:
        hs = TC.build(kind, sky)
        hs.textures = None
    if kind == "under_glass":
        return mapped(hs, [random_map(), GLASS_MAPS[glass_map]()], np.where(hs.tri_i32()[:, 0] == 0, 1, 0))
    return mapped(hs, [random_map()])


def arm(cosine=False):
    def sample(S, x, y, width, height, eye, cam, frame, trace=None):
        trace = trace if trace is not None else []
        out = normal_map_spec.sample(S, x, y, width, height, eye, cam, frame, trace)
        LEFT_OUT["samples"] += 1
        if "bssrdf-coplanar" in trace:
            LEFT_OUT["coplanar"] += 1
        elif "smooth-undecided" in trace:      # (tests/smooth_cases.py: compare_arm knows the one tag)
            LEFT_OUT["undecided"] += 1
            trace.append("bssrdf-coplanar")
        return out

    return types.SimpleNamespace(Scene=lambda hs, env_sampling=0, light_sampling=0: normal_map_spec.Scene(hs, env_sampling, light_sampling, cosine), sample=sample)


LEFT_OUT = {"coplanar": 0, "undecided": 0, "samples": 0}
SIZE, FRAMES = 12, tuple(range(8))
# texture_cases' cap, and 2 % more for samples whose mapped-normal decision - the tilt against zero, the bent normal's side - lies within
# the derived bound of a branch
LEFT_OUT_CAP = TC.LEFT_OUT_CAP + 0.02
# `need`: half of what the arm alone counts on these 1152 samples for the tags of this mode (count(); a sample counts once per tag)
CASES = {
    # the arm alone, 0 left out: 732 diffuse, 675 mapped, 67 mapped-culled, 2 mapped-side, 78 mapped-zero, 414 sky, 67 smooth-culled, 80 smooth-flat
    "diffuse": dict(need={"diffuse": 366, "mapped": 337, "mapped-culled": 33, "mapped-side": 1, "mapped-zero": 39, "sky": 207, "smooth-culled": 33, "smooth-flat": 40}),
    # the arm alone, 31 left out: 39 bssrdf, 646 diffuse, 650 mapped, 66 mapped-culled, 3 mapped-side, 83 mapped-zero, 414 sky, 66 smooth-culled, 83 smooth-flat, 90 sss
    "sss_diffuse": dict(need={"bssrdf": 19, "diffuse": 323, "mapped": 325, "mapped-culled": 33, "mapped-side": 1, "mapped-zero": 41, "sky": 207, "smooth-culled": 33, "smooth-flat": 41, "sss": 45}),
    # the arm alone, 25 left out: 45 bssrdf, 575 diffuse, 656 mapped, 54 mapped-culled, 3 mapped-side, 92 mapped-zero, 165 mirror, 414 sky, 54 smooth-culled, 95 smooth-flat, 12 smooth-redirect, 101 sss
    "jade": dict(need={"bssrdf": 22, "diffuse": 287, "mapped": 328, "mapped-culled": 27, "mapped-side": 1, "mapped-zero": 46, "mirror": 82, "sky": 207, "smooth-culled": 27, "smooth-flat": 47, "smooth-redirect": 6, "sss": 50}),
    # the arm alone, 0 left out: 316 diffuse, 679 mapped, 24 mapped-culled, 3 mapped-side, 74 mapped-zero, 570 mirror, 414 sky, 24 smooth-culled, 76 smooth-flat, 8 smooth-redirect
    "mirror_floor": dict(need={"diffuse": 158, "mapped": 339, "mapped-culled": 12, "mapped-side": 1, "mapped-zero": 37, "mirror": 285, "sky": 207, "smooth-culled": 12, "smooth-flat": 38, "smooth-redirect": 4}),
    # the arm alone, 0 left out: 637 diffuse, 693 mapped, 48 mapped-culled, 56 mapped-zero, 136 mirror, 145 refract, 414 sky, 48 smooth-culled, 56 smooth-flat, 5 smooth-redirect (the cube under its own 2 x 2 map: every refracted sample is mapped)
    "under_glass": dict(need={"diffuse": 318, "mapped": 346, "mapped-culled": 24, "mapped-zero": 28, "mirror": 68, "refract": 72, "sky": 207, "smooth-culled": 24, "smooth-flat": 28, "smooth-redirect": 2}),
    # the arm alone, 0 left out: 64 bssrdf, 563 diffuse, 657 mapped, 86 mapped-culled, 15 mapped-side, 101 mapped-zero, 157 mirror, 431 sky, 60 smooth, 90 smooth-culled, 46 smooth-flat, 17 smooth-redirect, 6 smooth-side, 110 sss
    "smooth_jade": dict(need={"bssrdf": 32, "diffuse": 281, "mapped": 328, "mapped-culled": 43, "mapped-side": 7, "mapped-zero": 50, "mirror": 78, "sky": 215, "smooth": 30, "smooth-culled": 45, "smooth-flat": 23, "smooth-redirect": 8, "smooth-side": 3, "sss": 55}),
    # the arm alone, 0 left out: 64 bssrdf, 563 diffuse, 657 mapped, 86 mapped-culled, 15 mapped-side, 101 mapped-zero, 157 mirror, 431 sky, 60 smooth, 90 smooth-culled, 46 smooth-flat, 17 smooth-redirect, 6 smooth-side, 110 sss, 715 textured
    "all_three": dict(need={"bssrdf": 32, "diffuse": 281, "mapped": 328, "mapped-culled": 43, "mapped-side": 7, "mapped-zero": 50, "mirror": 78, "sky": 215, "smooth": 30, "smooth-culled": 45, "smooth-flat": 23, "smooth-redirect": 8, "smooth-side": 3, "sss": 55, "textured": 357}),
}


def run(name, backend=None, out=None):
    c = CASES[name]
    for k in LEFT_OUT:
        LEFT_OUT[k] = 0
    res = SP.compare_arm(arm(), "mapped ", [], build, backend, name, SIZE, FRAMES, c["need"] if backend is not None else {}, out=out,
                         count_only=backend is None, max_left_out=LEFT_OUT_CAP)
    return res + (dict(LEFT_OUT),)


def count():
    """What the arm alone counts per case: python tests/normal_map_cases.py prints the tables the `need` entries above are half of."""
    for name in CASES:
        seen, _, n, skipped, left = run(name)
        print(name, n, skipped, left, dict(sorted(seen.items())), flush=True)


if __name__ == "__main__":
    count()
