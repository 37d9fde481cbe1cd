"""What the lens and the shutter tests share between their CPU and their GPU file: the cameras and camera moves, the rows the debug
entries are fed, hand-placed quads before the identity camera, and the poses, cases and expected samples of the shutter's
sample-for-sample comparison (from tests/shutter_spec.py, computed once per process); and the renders both modes are asked for on the
device in the same words: tinyjade close up, a scene with nothing in view, adaptive sampling and the denoiser on top."""
import os
import subprocess

import numpy as np

import jade_spec
import shutter_spec
from adaptive_ref import tile_errors
from conftest import ROOT, config_scene, tile_mask
from jaderaytracerendering_amd import _abi, backend as B, host as H
from render_helpers import same_bits, with_params
from spec_scenes import build

DEBUG_LIB = os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_hip_debug.so")
QUAD_I = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
IDENTITY_CAM = np.eye(4, dtype=np.float32).ravel()
LENS_ROW = 32  # floats per row of the debug entries: x, y, W, H, eye[3], cam[16], A, f, u1..u4, 3 unused (jade_debug_units.hip)
# floats per row of the debug entries (jade_debug_units.hip): the lens row's x, y, W, H, eye[3], cam[16], A, f, u1..u4, then ut, t_open,
# t_close, eye_close[3], cam_close[16], 13 unused
SHUTTER_ROW = 64


def exported(path):
    """The names a shared library defines."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def cameras():
    return [H.camera_orbit(2.8, 20.0, 10.0), H.camera_orbit(5.0, -35.0, 200.0, center=(0.3, -0.2, 1.0)), H.camera_orbit(1.2, 80.0, -60.0)]


def moves(eye, cam):
    """Close poses of (eye, cam): equal, a truck, an orbit about the origin, both, and a pan."""
    return [(eye.copy(), cam.copy()), H.camera_move(eye, cam, truck=(0.3, -0.1, 0.05)), H.camera_move(eye, cam, orbit_deg=4.0, pivot=(0, 0, 0)),
            H.camera_move(eye, cam, truck=(-0.05, 0.02, 0.0), orbit_deg=-6.0, pivot=(0.1, 0.0, -0.1)), H.camera_move(eye, cam, orbit_deg=3.0)]


def quad_scene(depth=3.0, half=1.0):
    """A quad across the axis of the identity camera (eye 0, looking down -z) at camera depth `depth`, a light behind the camera."""
    b = H.SceneBuilder()
    b.add_mesh(np.array([[-half, -half, -depth], [half, -half, -depth], [half, half, -depth], [-half, half, -depth]], np.float32), QUAD_I,
               H.material(brdf=(0.6, 0.5, 0.4)))
    b.add_mesh(np.array([[-1, -1, 4], [-1, 1, 4], [1, 1, 4], [1, -1, 4]], np.float32), QUAD_I, H.material(emissive=(5, 5, 5), brdf=(0.3, 0.3, 0.3)))
    b.set_env_constant(0.5, 0.6, 0.8)
    return b.build()


def emitter_on_the_axis(z, half=0.01):
    b = H.SceneBuilder()
    b.add_mesh(np.array([[-half, -half, -z], [half, -half, -z], [half, half, -z], [-half, half, -z]], np.float32), QUAD_I,
               H.material(emissive=(5, 5, 5), brdf=(0.3, 0.3, 0.3)))
    b.set_env_constant(0.0, 0.0, 0.0)
    return b.build()


def lens_rows(n_random=20000, seed=20):
    """float32 [n, LENS_ROW]: n_random random rows plus the edge rows - u3 and u4 at 0, 1.0f and 1 - 2^-24, the corner pixels, A over
    1e-4 .. 1, f over 0.1 .. 100."""
    rng = np.random.default_rng(seed)
    cams = cameras()
    rows = []

    def row(x, y, W, H_, cam_i, A, f, u):
        eye, cam = cams[cam_i]
        return np.concatenate([[x, y, W, H_], eye, cam, [A, f], u, [0, 0, 0]]).astype(np.float32)

    for _ in range(n_random):
        W, H_ = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        rows.append(row(int(rng.integers(0, W)), int(rng.integers(0, H_)), W, H_, int(rng.integers(0, 3)), 10.0 ** rng.uniform(-4, 0),
                        10.0 ** rng.uniform(-1, 2), rng.random(4).astype(np.float32)))
    ends = (0.0, 1.0, 1 - 2.0 ** -24)
    for W, H_ in ((64, 64), (40, 24), (1920, 1080)):
        for x, y in ((0, 0), (W - 1, 0), (0, H_ - 1), (W - 1, H_ - 1)):
            for A, f in ((1e-4, 0.1), (1e-4, 100.0), (1.0, 0.1), (1.0, 100.0), (0.1, 2.8)):
                for u3 in ends:
                    for u4 in ends:
                        for u1, u2 in ((0.0, 0.0), (1.0, 1.0)):
                            rows.append(row(x, y, W, H_, (x + y + len(rows)) % 3, A, f, (u1, u2, u3, u4)))
    return np.ascontiguousarray(np.stack(rows), dtype=np.float32)


def shutter_rows(n_random=6000, seed=21):
    """float32 [n, SHUTTER_ROW]: random rows - half of them under a lens, the close pose one of moves(), the interval random, now and
    then an instant - plus edge rows: ut, u3, u4 at 0, 1.0f and 1 - 2^-24, the corner pixels, equal poses, t_open == t_close."""
    rng = np.random.default_rng(seed)
    cams = cameras()
    closes = [moves(*c) for c in cams]
    rows = []

    def row(x, y, W, H_, cam_i, move_i, A, f, u, ut, t0, t1):
        eye, cam = cams[cam_i]
        eye_c, cam_c = closes[cam_i][move_i]
        return np.concatenate([[x, y, W, H_], eye, cam, [A, f], u, [ut, t0, t1], eye_c, cam_c, np.zeros(13)]).astype(np.float32)

    for i in range(n_random):
        W, H_ = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        lens = i % 2 == 1
        t0, t1 = np.sort(rng.random(2).astype(np.float32))
        if i % 7 == 0:
            t1 = t0
        if i % 11 == 0:
            t0, t1 = 0.0, 1.0
        rows.append(row(int(rng.integers(0, W)), int(rng.integers(0, H_)), W, H_, int(rng.integers(0, 3)), int(rng.integers(0, 5)),
                        10.0 ** rng.uniform(-4, 0) if lens else 0.0, 10.0 ** rng.uniform(-1, 2) if lens else 0.0, rng.random(4).astype(np.float32),
                        np.float32(rng.random()), t0, t1))
    ends = (0.0, 1.0, 1 - 2.0 ** -24)
    for W, H_ in ((64, 64), (40, 24), (1920, 1080)):
        for x, y in ((0, 0), (W - 1, 0), (0, H_ - 1), (W - 1, H_ - 1)):
            for A, f in ((0.0, 0.0), (1e-4, 100.0), (1.0, 0.1), (0.1, 2.8)):
                for ut in ends:
                    for u34 in ends:
                        for move_i in range(5):
                            for t0, t1 in ((0.0, 1.0), (0.5, 0.5), (0.0, 0.5)):
                                rows.append(row(x, y, W, H_, (x + y + len(rows)) % 3, move_i, A, f, (ut, 1.0 - ut, u34, u34), ut, t0, t1))
    return np.ascontiguousarray(np.stack(rows), dtype=np.float32)


# ------------------------------------------------------------------------------------------- the poses the shutter's GPU test renders --

SPEC_SIZE, SPEC_FRAMES = 12, (0, 1, 2)
SPEC_LENS = (0.1, 2.8)


def spec_poses():
    """The move of tests/test_gpu_shutter.py's sample-for-sample comparison: the orbit camera of tests/test_gpu_lens.py, an orbit of 4
    degrees about the scene's centre plus a small truck, the whole move exposed."""
    eye, cam = H.camera_orbit(2.8, 20.0, 10.0)
    eye_c, cam_c = H.camera_move(eye, cam, truck=(0.05, -0.03, 0.0), orbit_deg=4.0, pivot=(0.0, 0.0, 0.0))
    return eye, cam, (eye_c, cam_c, 0.0, 1.0)


# by case: (scene kind, sky, env_sampling, lens or None) - tests/test_gpu_shutter.py renders these
SPEC_CASES = {
    "jade_cube": ("jade_cube", False, _abi.ENV_REFERENCE, None),
    "glass_cube": ("glass_cube", False, _abi.ENV_REFERENCE, None),
    "open_floor": ("open_floor", False, _abi.ENV_REFERENCE, None),
    "jade_cube-lens": ("jade_cube", False, _abi.ENV_REFERENCE, SPEC_LENS),
    "jade_cube-importance": ("jade_cube", True, _abi.ENV_IMPORTANCE, None),
}
# What shutter_spec.sample alone counts per branch on those pixels (432 samples a case; bssrdf-coplanar samples left out, their number
# under "left-out"): tests/test_shutter_cpu.py's test_the_spec_s_own_branch_counts recounts them, on the CPU; tests/test_gpu_shutter.py
# asks for half of each among the samples on which the device agrees.
SPEC_COUNTS = {
    "jade_cube": {"bssrdf": 15, "diffuse": 222, "mirror": 65, "sky": 152, "sss": 38, "left-out": 13},
    "glass_cube": {"diffuse": 239, "mirror": 57, "refract": 56, "refract-open": 10, "sky": 152, "left-out": 0},
    "open_floor": {"diffuse": 237, "sky": 193, "left-out": 0},
    "jade_cube-lens": {"bssrdf": 12, "diffuse": 220, "mirror": 57, "sky": 153, "sss": 41, "left-out": 9},
    "jade_cube-importance": {"bssrdf": 17, "diffuse": 225, "env-importance": 183, "env-noenv": 89, "mirror": 63, "sky": 152, "sss": 38, "left-out": 11},
}


def spec_samples(case):
    """[(frame, x, y, want[3], trace)] of a case, from shutter_spec.sample - computed once and shared (tests/test_gpu_shutter.py)."""
    if case not in _spec_cache:
        kind, sky, env_sampling, lens = SPEC_CASES[case]
        S = jade_spec.Scene(build(kind, sky), env_sampling)
        eye, cam, shutter = spec_poses()
        A, f = lens if lens else (0.0, 0.0)
        out = []
        for frame in SPEC_FRAMES:
            for y in range(SPEC_SIZE):
                for x in range(SPEC_SIZE):
                    tr = []
                    want = shutter_spec.sample(S, x, y, SPEC_SIZE, SPEC_SIZE, eye, cam, frame, A, f, shutter, tr)
                    out.append((frame, x, y, want, tr))
        _spec_cache[case] = out
    return _spec_cache[case]


_spec_cache = {}


# ------------------------------------------------------------------------------- what the lens and the shutter tests render on the device --

def wang(s):
    """One step of jade_wang (include/jade_fpmath.h) on a Python int."""
    s = ((s ^ 61) ^ (s >> 16)) & 0xffffffff
    s = (s * 9) & 0xffffffff
    s = s ^ (s >> 4)
    s = (s * 0x27d4eb2d) & 0xffffffff
    return s ^ (s >> 15)


def tinyjade(spp, w=40, h=24):
    """(host scene, parameters, a close pose for the shutter).  40 x 24: partial tiles; at 64 spp 960 x 64 records: more than one
    512-thread block, a last wave partly filled."""
    hs, cfg = config_scene("tinyjade")
    p = B.params_from_config(cfg, spp=spp)
    p.width, p.height = w, h
    eye, cam = np.array(p.eye[:], np.float32), np.array(p.camera[:], np.float32)
    # the statuette is about 0.45 away: a turntable step of 3 degrees about the orbit's centre and a small truck
    close = H.camera_move(eye, cam, truck=(0.004, -0.002, 0.0), orbit_deg=3.0, pivot=(0.26, -1.28, 0.0))
    return hs, p, close


def nothing_in_view():
    """The geometry is behind the identity camera and the sky one constant.  The constant lies ABOVE the lookup's clamp at 10
    (PathTrace.cu:694-702): the bilinear lookup of a constant map returns it only up to an ulp that depends on the direction (four
    weights that add up to 1 +- 2^-24), and the clamp makes (10, 10, 10) of every such value - so that every sample of a frame is the
    same constant bit for bit, whatever its ray."""
    b = H.SceneBuilder()
    b.add_mesh(np.array([[-1, -1, 4], [-1, 1, 4], [1, 1, 4], [1, -1, 4]], np.float32), QUAD_I, H.material(emissive=(5, 5, 5), brdf=(0.3, 0.3, 0.3)))
    b.add_mesh(np.array([[-1, -1, 3], [1, -1, 3], [1, 1, 3], [-1, 1, 3]], np.float32), QUAD_I, H.material(brdf=(0.6, 0.5, 0.4)))
    b.set_env_constant(20.0, 30.0, 40.0)
    return b.build()


def check_adaptive_tiles_equal_uniform_renders(hip, prepare):
    """Under the camera mode prepare(sc) sets, every tile of an adaptive render is the uniform render of its sample count, bit for bit."""
    hs, p, _ = tinyjade(16, 64, 48)
    floor = 0.01
    with hip.scene(hs) as sc:
        prepare(sc)
        sc.begin(with_params(p, spp=2))
        sc.step(2)
        e = np.sort(tile_errors(sc.error_map(floor), 4, 3).ravel())
        e = e[np.isfinite(e)]
        rel = next(float(0.5 * (e[i] + e[i + 1])) for i in range(len(e) // 2, len(e) - 1) if e[i + 1] > e[i] * (1 + 1e-3))
        rgb, bgr, tspp, st = sc.render_adaptive(p, 2, rel, floor)
        ks = sorted(set(tspp.ravel().tolist()))
        assert len(ks) >= 2 and st.rays_inline == 0, ks
        for k in ks:
            r_u, b_u, _ = sc.render(with_params(p, spp=int(k)))
            m = tile_mask(p.width, p.height, np.flatnonzero(tspp.ravel() == k))
            assert same_bits(rgb[m], r_u[m]) and np.array_equal(bgr[m], b_u[m]), k
    assert st.samples == int(tspp.sum()) * 256


def check_denoise_is_denoise_image_on_its_own_inputs(hip, prepare):
    hs, p, _ = tinyjade(16)
    d = hip.denoise_defaults()
    with hip.scene(hs) as sc:
        prepare(sc)
        sc.begin(p)
        sc.step(16)
        r1, b1 = sc.denoise(d)
        g = sc.guides(d.guide_spp)
        rgb, _ = sc.resolve(want_bgr8=False)
    got = hip.denoise_image(rgb, g["variance"], g["albedo"], g["normal"], g["depth"], params=d)
    assert same_bits(got, r1) and np.isfinite(r1).all()
