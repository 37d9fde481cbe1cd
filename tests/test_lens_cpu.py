"""The thin-lens camera without a GPU (include/jade_bvh.h, "The lens, stated").

tests/lens_spec.py states the lens ray in float64; here that statement is first rested on something other than itself - geometry:
every lens ray of a jitter meets the pinhole ray of that jitter in the plane of focus (a), a point off that plane is seen through a
disk of image positions whose radius has a closed form (b), the lens points cover the disk uniformly (c) - and then the module's fp32
evaluation (lens_ray, jade_device.h, compiled for the host: jade_debug_lens_ray_host of libjade_hip_debug.so, no HIP call) is held
against it under a bound derived from its roundings (d).  Then the ABI (e), the command line's flags (f) and autofocus (g).
tests/test_gpu_lens.py compares the device with the same rows and the render with lens_spec.sample."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lens_spec
from camera_cases import DEBUG_LIB, IDENTITY_CAM, QUAD_I, cameras, exported, lens_rows, quad_scene
from conftest import B, ORACLE_LIB, ROOT
from jaderaytracerendering_amd import _abi, host as H
from render_helpers import CLI

DEBUG_ENTRIES = ("jade_debug_lens_ray_host", "jade_debug_lens_ray", "jade_debug_lens_ray_rng")


# ------------------------------------------------------------------------------------------------------------------ (a) focus --

@pytest.mark.parametrize("W,H_", [(32, 32), (40, 24)])
def test_every_lens_ray_meets_the_pinhole_ray_in_the_plane_of_focus(W, H_):
    g = np.array([0.0, 1.0, 0.25, 0.5, 0.75, 0.1, 0.9, 0.6])
    u3, u4 = (v.ravel() for v in np.meshgrid(g, g))  # 64 lens points, u3 and u4 at 0 and at 1 among them
    for eye, cam in cameras():
        for A, f in ((0.1, 2.8), (1.0, 0.1), (1e-4, 100.0)):
            for x, y in ((0, 0), (W - 1, 0), (0, H_ - 1), (W - 1, H_ - 1), (W // 2, H_ // 3)):
                for u1, u2 in ((0.0, 0.0), (1.0, 1.0), (0.5, 0.5), (0.3, 0.8)):
                    left, up = lens_spec.offsets(x, y, W, H_, u1, u2)
                    k = f / 1.5
                    pf = np.asarray(eye, np.float64) + lens_spec.transform(np.array([left * k, up * k, -1.5 * k]), cam)
                    _, dp = lens_spec.pinhole_ray(x, y, W, H_, eye, cam, u1, u2)
                    w = pf - np.asarray(eye, np.float64)
                    assert np.abs(w - (w @ dp) * dp).max() <= 1e-12 * f, "the pinhole ray's own point"
                    o, d = lens_spec.ray(x, y, W, H_, eye, cam, A, f, u1, u2, u3, u4)
                    w = pf - o
                    miss = w - (w * d).sum(-1)[:, None] * d
                    assert np.sqrt((miss * miss).sum(-1)).max() <= 1e-12 * f
                    # the plane of focus is camera-space z = -f: the lens rays reach pf going forward
                    assert ((w * d).sum(-1) > 0).all()
                    centre = u3 == 0.0
                    assert centre.sum() == 8 and (o[centre] == np.asarray(eye, np.float64)).all(), "u3 = 0: the origin is the eye, exactly"


# ------------------------------------------------------------------------------------------------------ (b) circle of confusion --

@pytest.mark.parametrize("W,H_", [(32, 32), (40, 24)])
def test_circle_of_confusion_closed_form(W, H_):
    """A point Q at camera depth z is seen from lens point (lx, ly) through the image-plane position of the pinhole displaced by
    1.5 (lx, ly) (1/f - 1/z): in pixels (one pixel = 2/H of the plane, both axes) 0.75 H (lx, ly) (1/f - 1/z), a disk of radius
    0.75 H A |1/z - 1/f|."""
    eye, cam = cameras()[0]
    A, f = 0.1, 2.8
    g = (np.arange(8) + 0.5) / 8
    u3, u4 = (v.ravel() for v in np.meshgrid(np.concatenate([g, [1.0]]), g))
    for z in (f / 2, f, 2 * f, 10 * f):
        for qx, qy in ((0.0, 0.0), (0.21 * z, -0.13 * z)):  # camera-space (qx, qy, -z): inside the frame of both shapes
            Q = np.asarray(eye, np.float64) + lens_spec.transform(np.array([qx, qy, -z]), cam)
            # the pinhole sees Q at the plane position (1.5 qx / z, 1.5 qy / z); as continuous pixel coordinates (x + u1, y + u2):
            px0 = (1.5 * qx / z / (W / H_) + 1) * W / 2 + 0.5
            py0 = (1.5 * qy / z + 1) * H_ / 2 + 0.5
            lx, ly = lens_spec.lens_point(A, u3, u4)
            px = px0 + 0.75 * H_ * lx * (1 / f - 1 / z)
            py = py0 + 0.75 * H_ * ly * (1 / f - 1 / z)
            x, y = np.floor(px), np.floor(py)
            assert (x >= 0).all() and (x < W).all() and (y >= 0).all() and (y < H_).all()
            o, d = lens_spec.ray(x, y, W, H_, eye, cam, A, f, px - x, py - y, u3, u4)
            w = Q - o
            miss = w - (w * d).sum(-1)[:, None] * d
            assert np.sqrt((miss * miss).sum(-1)).max() <= 1e-12 * z, (z, qx)
            r_px = np.sqrt((px - px0) ** 2 + (py - py0) ** 2)
            R = 0.75 * H_ * A * abs(1 / z - 1 / f)
            assert r_px.max() <= R * (1 + 1e-12) + 1e-12
            assert abs(r_px[u3 == 1.0].min() - R) <= 1e-12 * max(R, 1.0), "the rim of the lens draws the rim of the disk"
            if z == f:
                assert r_px.max() == 0.0


# -------------------------------------------------------------------------------------------------------------- (c) lens points --

def test_lens_points_cover_the_disk_uniformly():
    """On the 64 x 64 stratified grid (u3, u4) = ((i + 1/2) / 64, (j + 1/2) / 64): r^2 = lx^2 + ly^2 = A^2 u3 (cos^2 + sin^2), LINEAR
    in u3, so the midpoint rule has no discretisation error at all: mean u3 = (1/64) sum (i + 1/2) / 64 = 1/2 exactly, and
    E[r^2] = A^2 / 2 up to float64 rounding.  That rounding, in units of 2^-53 relative: sqrt 1, A * sqrt 1 (doubled by the square:
    4), cos and sin 1 each and the products r cs, r sn 1 each (doubled by the squares: 4), the two squares and their sum 2, numpy's
    pairwise mean of 4096 terms log2(4096) = 12, its division 1: 23, asserted as 32 * 2^-53.  (Uniform over the disk means the area
    inside radius r grows as r^2: E[r^2] = A^2 / 2, against A^2 / 3 for a radius drawn uniformly.)"""
    g = (np.arange(64) + 0.5) / 64
    u3, u4 = (v.ravel() for v in np.meshgrid(g, g))
    for A in (1e-4, 0.1, 1.0):
        lx, ly = lens_spec.lens_point(A, u3, u4)
        r2 = lx * lx + ly * ly
        assert abs(r2.mean() - A * A / 2) <= 32 * 2.0 ** -53 * A * A / 2
        assert (np.sqrt(r2) <= A * (1 + 4 * 2.0 ** -53)).all()
    # and at the ends of both draws: r <= A, the rim reached at u3 = 1
    e = np.array([0.0, 1.0, 1 - 2.0 ** -24])
    u3, u4 = (v.ravel() for v in np.meshgrid(e, e))
    lx, ly = lens_spec.lens_point(0.1, u3, u4)
    assert (np.sqrt(lx * lx + ly * ly) <= 0.1 * (1 + 4 * 2.0 ** -53)).all()


# ------------------------------------------------------------------------------------------------------- (d) fp32 against float64 --

def lens_rows_spec(rows):
    """lens_spec.ray on the rows (float64 from the rows' float32 values) -> origin [n, 3], dir [n, 3]."""
    r = rows.astype(np.float64)
    return lens_spec.ray(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4:7], r[:, 7:23], r[:, 23], r[:, 24], r[:, 25], r[:, 26], r[:, 27], r[:, 28])


def lens_rows_bound(rows):
    """The bound of test_fp32_lens_ray_against_the_statement, per row: (D_origin relative to |eye| + A, D_dir per component)."""
    r = rows.astype(np.float64)
    e = 2.0 ** -24
    S = 2.5e-7 + 2 * lens_spec.PI * e
    A, f = r[:, 23], r[:, 24]
    k = f / 1.5
    left, up = lens_spec.offsets(r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 25], r[:, 26])
    m = np.maximum(np.maximum(np.abs(left), np.abs(up)), 1.5)
    cam = np.abs(r[:, 7:23])
    M1 = np.max(np.stack([cam[:, rr] + cam[:, 4 + rr] + cam[:, 8 + rr] for rr in range(3)], -1), -1)
    E_L = A * (S + 4 * e)
    e_j = 2.0 / r[:, 3] * e * np.maximum(r[:, 0] + 1, r[:, 1] + 1)
    e_c = (5 * e * m + e_j) * k + E_L + e * A
    lx, ly = lens_spec.lens_point(A, r[:, 27], r[:, 28])
    d_c = np.stack([left * k - lx, up * k - ly, -1.5 * k], -1)
    v = lens_spec.transform(d_c, r[:, 7:23])
    e_v = M1 * (4 * e * np.abs(d_c).max(-1) + e_c)
    D_dir = 2 * np.sqrt(3.0) * e_v / np.sqrt((v * v).sum(-1)) + 6 * e
    eye = np.abs(r[:, 4:7]).max(-1)
    D_org = (M1 * (E_L + 4 * e * A) + e * (eye + M1 * A) * (1 + e)) / (eye + A)
    return D_org, D_dir


@pytest.fixture(scope="module")
def debug_lib():
    assert os.path.exists(DEBUG_LIB), "libjade_hip_debug.so missing: run `make hipvariants` (or __graft_entry__.build())"
    lib = ctypes.CDLL(DEBUG_LIB)
    lib.jade_debug_lens_ray_host.restype = ctypes.c_int
    lib.jade_debug_lens_ray_host.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_fp32_lens_ray_against_the_statement(debug_lib):
    """lens_ray compiled for the host against lens_spec.ray on > 20 000 rows.  The bound, from the roundings of the statement, with
    e = 2^-24 (one fp32 operation: x (1 + d), |d| <= e), first order, every count of e raised by one for the second-order terms:

      S   = 2.5e-7 + 2 PI e     jade_sincosf's error (tests/test_fpmath.py's bound, absolute) plus that of its argument: phi is one
                                product with the exact constant fl(2 PI), off by at most 2 PI e
      r   = A sqrt(u3): a correctly rounded root and a product                                   |dr| <= 2 e A
      lx, ly = r cs, r sn: |dlx| <= A S + dr + e A                                               E_L = A (S + 4 e)
      k   = f / 1.5f: one division, e k
      left_offset, up_offset: the pixel's coordinate plus its jitter, fx = x + u1 and fy = y + u2, is ONE fp32 addition, off by
            e (x + 1) and e (y + 1); the plane's 2 / H per pixel (both axes: 2 / W times W / H) makes of it
            e_j = (2 / H) e max(x + 1, y + 1); the rest is float64 (the statement's own arithmetic up to 2^-52) rounded once to fp32,
            e m with m = max(|left_offset|, |up_offset|, 1.5)
      d_c = (left_offset k - lx, up_offset k - ly, -1.5 k): the product carries (3 e m + e_j) k, the subtraction adds E_L and rounds
            once, e (m k + A)                                                                    e_c = (5 e m + e_j) k + E_L + e A
      v   = jade_transform(d_c, 0, cam): per component a sum of three products, one rounding each (the fourth, m * 0, adds +0
            exactly): 3 e M1 |d_c|_inf on its own, M1 e_c from its input, M1 = the largest sum of |cam| over a row of the rotation
            (<= sqrt 3)                                                                          e_v = M1 (4 e |d_c|_inf + e_c)
      dir = v / |v|: the perturbation of a normalised vector is at most 2 |dv|_2 / |v| <= 2 sqrt(3) e_v / |v|; the scale itself -
            a dot product of non-negative terms (3 e, halved by the root), the root, the reciprocal, the product - 4.5 e
                                                                                                 D_dir = 2 sqrt(3) e_v / |v| + 6 e
      origin = eye + jade_transform((lx, ly, 0), 0, cam): M1 E_L from the lens point, 3 e M1 A from the sums, e (|eye|_inf + M1 A)
            from the addition; relative to |eye|_inf + A         D_org = (M1 (E_L + 4 e A) + e (|eye|_inf + M1 A)) / (|eye|_inf + A)

    D_dir is dominated by A S / (1.5 k) = A S / f: an aperture as wide as the focus distance turns the sine's 2.5e-7 into as much
    of the direction.  The measured worst case is in DESIGN.md 3.9."""
    rows = lens_rows()
    assert len(rows) >= 20000
    out = np.zeros((len(rows), 6), np.float32)
    assert debug_lib.jade_debug_lens_ray_host(len(rows), rows.ctypes.data, out.ctypes.data) == 0
    o, d = lens_rows_spec(rows)
    D_org, D_dir = lens_rows_bound(rows)
    r = rows.astype(np.float64)
    err_d = np.abs(out[:, 3:].astype(np.float64) - d).max(-1)
    err_o = np.abs(out[:, :3].astype(np.float64) - o).max(-1) / (np.abs(r[:, 4:7]).max(-1) + r[:, 23])
    print(f"lens ray fp32 vs float64 over {len(rows)} rows: dir worst {err_d.max():.3g} (bound there {D_dir[err_d.argmax()]:.3g}, "
          f"worst ratio {np.max(err_d / D_dir):.3g}); origin worst {err_o.max():.3g} relative (worst ratio {np.max(err_o / D_org):.3g})")
    i = int(np.argmax(err_d / D_dir))
    assert (err_d <= D_dir).all(), (i, rows[i], err_d[i], D_dir[i])
    i = int(np.argmax(err_o / D_org))
    assert (err_o <= D_org).all(), (i, rows[i], err_o[i], D_org[i])
    assert np.isfinite(out).all()
    # u3 = 0: the eye itself, in fp32 too
    centre = rows[:, 27] == 0.0
    assert centre.any() and (out[centre, :3] == rows[centre, 4:7]).all()


# ------------------------------------------------------------------------------------------------------------------------ (e) ABI --

def test_abi():
    assert ctypes.sizeof(_abi.LensParams) == 8
    assert [(n, getattr(_abi.LensParams, n).offset) for n, _ in _abi.LensParams._fields_] == [("aperture_radius", 0), ("focus_distance", 4)]
    text = open(os.path.join(ROOT, "include", "jade_rt.h")).read()
    assert int(re.search(r"#define JADE_ABI_VERSION (\d+)", text).group(1)) == 7 and "lens" not in text.lower()
    bvh = open(os.path.join(ROOT, "include", "jade_bvh.h")).read()
    assert "typedef struct jade_lens_params" in bvh and "The lens, stated" in bvh
    hip, dbg, orc = exported(B.HIP_LIB), exported(DEBUG_LIB), exported(ORACLE_LIB)
    for name in ("jade_scene_set_lens", "jade_scene_get_lens"):
        assert name in hip and name in dbg and name not in orc, name
        assert name in _abi.BVH_SYMBOLS
    for name in DEBUG_ENTRIES:
        assert name in dbg and name not in hip, name
    assert "jadeh_focus_distance" in exported(os.path.join(ROOT, "jaderaytracerendering_amd", "lib", "libjade_host.so"))


def test_the_oracle_has_no_lens(oracle):
    hs = quad_scene()
    with oracle.scene(hs) as so:
        for call in (lambda: so.set_lens(0.1, 2.0), so.lens):
            with pytest.raises(B.JadeError) as ei:
                call()
            assert ei.value.code == _abi.JADE_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------------ (f) CLI --

@pytest.mark.parametrize("flags", [
    ["--aperture"], ["--aperture", "wide", "--focus", "2"], ["--aperture", "nan", "--focus", "2"], ["--aperture", "-0.1", "--focus", "2"],
    ["--aperture", "0.1"], ["--aperture", "0.1", "--focus"], ["--aperture", "0.1", "--focus", "0"], ["--aperture", "0.1", "--focus", "-2"],
    ["--aperture", "0.1", "--focus", "inf"], ["--aperture", "0.1", "--focus", "1e60"], ["--aperture", "0.1", "--focus", "2", "--focus-at", "3,4"],
    ["--aperture", "0.1", "--focus-at"], ["--aperture", "0.1", "--focus-at", "3"], ["--aperture", "0.1", "--focus-at", "3,"],
    ["--aperture", "0.1", "--focus-at", "-1,4"], ["--aperture", "0.1", "--focus-at", "1.5,4"], ["--aperture", "0.1", "--focus-at", "3,x"],
    ["--aperture", "0.1", "--focus-at", "32,4", "--width", "32", "--height", "32"],
    ["--focus", "2"], ["--focus-at", "3,4"],
], ids=lambda f: " ".join(f))
def test_cli_rejects_malformed_lens_flags_before_building_a_scene(flags, tmp_path):
    r = subprocess.run([CLI, "--config", "tiny", "--backend", ORACLE_LIB, *flags], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr, (r.returncode, r.stderr)
    assert "Start..." not in r.stdout


def test_cli_on_the_oracle_refuses_the_aperture(tmp_path):
    r = subprocess.run([CLI, "--config", "tiny", "--width", "32", "--height", "32", "--spp", "2", "--backend", ORACLE_LIB, "--aperture", "0.1",
                        "--focus", "2.5", "--out", "o.ppm"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 2 and "--aperture needs the HIP backend" in r.stderr, (r.returncode, r.stderr)
    assert not os.path.exists(tmp_path / "o.ppm")


# ------------------------------------------------------------------------------------------------------------------ (g) autofocus --

def test_focus_distance_against_a_hand_placed_quad(oracle):
    """The quad at depth 3 fills |x|, |y| <= 1: the image plane sits at 1.5, so it shows on plane positions |left|, |up| <= 0.5 - the
    middle half of a square frame.  Every pixel of it focuses at 3 (the depth along the axis, not the distance along the ray: the
    ray of pixel (20, 40) is 3.13 long); the fp32 triangle test and one division leave a few 2^-24 of 3."""
    W = 64
    p = B.make_params(W, W, 1, (0, 0, 0), IDENTITY_CAM)
    with oracle.scene(quad_scene(3.0)) as so:
        for px, py in ((33, 32), (30, 31), (20, 40), (47, 16), (16, 47)):  # (off the quad's diagonal: the triangle test is strict)
            f = so.focus_distance(p, px, py)
            assert abs(f - 3.0) <= 16 * 2.0 ** -24 * 3.0, (px, py, f)
        for px, py in ((0, 0), (63, 63), (10, 32), (32, 50)):  # beside the quad: the sky
            with pytest.raises(RuntimeError, match="sees no surface"):
                so.focus_distance(p, px, py)
        for px, py in ((-1, 0), (64, 0), (0, 64)):
            with pytest.raises(RuntimeError, match="outside the frame"):
                so.focus_distance(p, px, py)
    with oracle.scene(quad_scene(0.75, 0.2)) as so:
        assert abs(so.focus_distance(p, 33, 32) - 0.75) <= 16 * 2.0 ** -24 * 0.75
    # a turned camera: the orbit camera looks at the origin from 2.8 away; a quad through the origin facing it is 2.8 deep
    eye, cam = H.camera_orbit(2.8, 20.0, 10.0)
    b = H.SceneBuilder()
    M = np.asarray(cam, np.float64).reshape(4, 4)
    right, upv = M[0][:3], M[1][:3]
    v = np.array([-right - upv, right - upv, right + upv, -right + upv], np.float32)
    b.add_mesh(v, QUAD_I, H.material(brdf=(0.6, 0.5, 0.4)))
    b.add_mesh(np.array([[-1, 5, -1], [-1, 5, 1], [1, 5, 1], [1, 5, -1]], np.float32), QUAD_I, H.material(emissive=(5, 5, 5), brdf=(0.3, 0.3, 0.3)))
    b.set_env_constant(0.5, 0.6, 0.8)
    with oracle.scene(b.build()) as so:
        p = B.make_params(40, 24, 1, eye, cam)
        for px, py in ((21, 12), (14, 7), (24, 15)):
            assert abs(so.focus_distance(p, px, py) - 2.8) <= 32 * 2.0 ** -24 * 2.8, (px, py)
