"""The camera shutter on the device (include/jade_bvh.h, "The shutter, stated"; jade_scene_set_shutter): the shutter ray against its
host build, no shutter against a handle that never heard of one, the render sample for sample against tests/shutter_spec.py, hard
geometric bounds on the streak of a truck, and the entry points that begin a render or read one - adaptive sampling, the guides and the
denoiser, the command line.  The seams every mode is held to - twice, the walks, steps, tile shares, schedules, jade_render_multi - are
in tests/test_gpu_mode_seams.py (cases "shutter" and "shutter+lens" of tests/mode_seams.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import camera_cases as CC
import jade_spec
import mode_seams as MS
import shutter_spec
from conftest import B, config_scene
from jaderaytracerendering_amd import _abi, host as H
from render_helpers import CLI, SCHED_LENS, all_counters, read_pfm, same_bits
from spec_scenes import build

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1. the shutter ray, device = host --

def test_shutter_ray_device_equals_host_build_bit_for_bit(hip_debug):
    lib = hip_debug.lib
    for fn in (lib.jade_debug_shutter_ray_host, lib.jade_debug_shutter_ray, lib.jade_debug_shutter_ray_rng):
        fn.restype = ctypes.c_int
    lib.jade_debug_shutter_ray_host.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.jade_debug_shutter_ray.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    rows = CC.shutter_rows()
    host = np.zeros((len(rows), 6), np.float32)
    dev = np.full((len(rows), 6), np.nan, np.float32)
    hip_debug.check(lib.jade_debug_shutter_ray_host(len(rows), rows.ctypes.data, host.ctypes.data))
    hip_debug.check(lib.jade_debug_shutter_ray(0, len(rows), rows.ctypes.data, dev.ctypes.data))
    bad = np.flatnonzero((host.view(np.uint32) != dev.view(np.uint32)).any(-1))
    assert len(bad) == 0, (len(bad), rows[bad[0]], host[bad[0]], dev[bad[0]])

    # from the stream: the draws in the stated order, and the state exactly three (no lens) or five (lens) Wang steps on
    lib.jade_debug_shutter_ray_rng.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_float, ctypes.c_float, ctypes.POINTER(_abi.ShutterParams)] + [ctypes.c_void_p] * 5
    W, H_, frame = 40, 24, 7
    eye, cam, (eye_c, cam_c, _, _) = CC.spec_poses()
    t0, t1 = 0.25, 0.75
    sh = _abi.ShutterParams(_abi.f3(*eye_c.tolist()), (ctypes.c_float * 16)(*cam_c.tolist()), t0, t1)
    ys, xs = (v.ravel().astype(np.int32) for v in np.mgrid[0:H_, 0:W])
    sidx = ((xs * 7 + ys * 13) % 1500).astype(np.uint32)
    n = len(xs)
    for A, f in ((0.0, 0.0), (0.1, 2.8)):
        out = np.zeros((n, 6), np.float32)
        state = np.zeros(n, np.uint32)
        hip_debug.check(lib.jade_debug_shutter_ray_rng(0, n, W, H_, frame, eye.ctypes.data, cam.ctypes.data, A, f, ctypes.byref(sh), xs.ctypes.data,
                                                       ys.ctypes.data, sidx.ctypes.data, out.ctypes.data, state.ctypes.data))
        rows2 = np.zeros((n, CC.SHUTTER_ROW), np.float32)
        want_state = np.zeros(n, np.uint32)
        for i in range(n):
            s = ((int(xs[i]) * 1973 + int(ys[i]) * 9277 + (frame + int(sidx[i])) * 26699) | 1) & 0xffffffff
            u = []
            for _ in range(5 if A > 0 else 3):  # jade_wang, include/jade_fpmath.h
                s = CC.wang(s)
                u.append(np.float32(s) * np.float32(2.0 ** -32))
            want_state[i] = s
            u1, u2, u3, u4, ut = u if A > 0 else (u[0], u[1], 0.0, 0.0, u[2])
            rows2[i] = np.concatenate([[xs[i], ys[i], W, H_], eye, cam, [A, f, u1, u2, u3, u4, ut, t0, t1], eye_c, cam_c, np.zeros(13)]).astype(np.float32)
        assert np.array_equal(state, want_state), A
        host2 = np.zeros((n, 6), np.float32)
        hip_debug.check(lib.jade_debug_shutter_ray_host(n, rows2.ctypes.data, host2.ctypes.data))
        assert same_bits(out, host2), A


# -------------------------------------------------------------------------------------------- 2. no shutter is today's render --

def test_no_shutter_is_the_render_of_a_handle_that_never_had_one_in_every_bit_and_counter(hip):
    hs, p, close = CC.tinyjade(24)
    lens = SCHED_LENS
    with hip.scene(hs) as sc:
        ref_pin = sc.render(p)
        assert sc.shutter() is None
        sc.set_lens(*lens)
        ref_lens = sc.render(p)
    assert ref_pin[2].rays_inline > 0, "the fused first pass runs"

    def check(prepare, ref):
        with hip.scene(hs) as sc:
            prepare(sc)
            rgb, bgr, st = sc.render(p)
        assert same_bits(rgb, ref[0]) and np.array_equal(bgr, ref[1])
        assert all_counters(st) == all_counters(ref[2])

    check(lambda sc: sc.set_shutter(None), ref_pin)
    check(lambda sc: (sc.set_shutter(*close), sc.set_shutter(None)), ref_pin)
    check(lambda sc: (sc.set_lens(*lens), sc.set_shutter(None)), ref_lens)
    check(lambda sc: (sc.set_shutter(*close, 0.25, 0.5), sc.set_lens(*lens), sc.set_shutter(None)), ref_lens)

    eye, cam = np.array(p.eye[:], np.float32), np.array(p.camera[:], np.float32)
    with hip.scene(hs) as sc:
        sc.set_shutter(*close, 0.25, 0.75)
        got = sc.shutter()
        assert np.array_equal(got[0], close[0]) and np.array_equal(got[1], close[1]) and got[2:] == (0.25, 0.75)
        nan_eye, inf_cam = close[0].copy(), close[1].copy()
        nan_eye[1] = np.nan
        inf_cam[14] = np.inf  # (all 16 floats of the matrix are checked, also those the ray does not read)
        for bad in ((nan_eye, close[1]), (close[0], inf_cam), (close[0], close[1], -0.1, 0.5), (close[0], close[1], 0.6, 0.5), (close[0], close[1], 0.0, 1.5),
                    (close[0], close[1], np.nan, 1.0), (close[0], close[1], 0.0, np.nan), (close[0], close[1], 0.0, np.inf)):
            with pytest.raises(B.JadeError) as ei:
                sc.set_shutter(*bad)
            assert ei.value.code == _abi.JADE_ERR_INVALID, bad
            got = sc.shutter()
            assert np.array_equal(got[0], close[0]) and np.array_equal(got[1], close[1]) and got[2:] == (0.25, 0.75), "an invalid shutter leaves the previous one"
        blurred = sc.render(p)
        # a render in progress keeps the shutter it began with: unset between two steps, the frame is the one-call shutter frame
        sc.begin(p)
        sc.step(12)
        sc.set_shutter(None)
        sc.step(12)
        rgb2, bgr2 = sc.resolve()
        # the mode is entered even for equal poses: the time's draw is taken, so the samples are other samples of the same image
        sc.set_shutter(eye, cam)
        still = sc.render(p)
    assert not same_bits(blurred[0], ref_pin[0])
    assert same_bits(rgb2, blurred[0]) and np.array_equal(bgr2, blurred[1])
    assert still[2].rays_inline == 0 and still[2].samples == ref_pin[2].samples and not same_bits(still[0], ref_pin[0])


# ----------------------------------------------------------------------------------- 3. sample for sample against the statement --

@pytest.mark.parametrize("case", sorted(CC.SPEC_CASES))
def test_render_matches_the_float64_statement_sample_for_sample(hip, case):
    """tests/test_gpu_lens.py's settings (size 12, frames 0-2, spp 1) and rule - a sample agrees when every channel is within
    1e-4 max(|want|, 1e-3); at most 2 % may disagree (a cap: a decision fp32 and float64 take differently, such as a ray grazing an
    edge); bssrdf-coplanar samples are left out as there.  Per branch, at least half of what the statement alone counts
    (tests/test_shutter_cpu.py, SPEC_COUNTS) must be among the agreeing samples.  Disagreeing samples on the MI355X at the time of
    writing: DESIGN.md 3.10."""
    kind, sky, env_sampling, lens = CC.SPEC_CASES[case]
    hs = build(kind, sky)
    eye, cam, shutter = CC.spec_poses()
    size = CC.SPEC_SIZE
    frames = {}
    with hip.scene(hs) as sc:
        if lens:
            sc.set_lens(*lens)
        sc.set_shutter(*shutter)
        for frame in CC.SPEC_FRAMES:
            p = B.make_params(size, size, 1, eye, cam, frame=frame, env_sampling=env_sampling)
            rgb, _, st = sc.render(p, want_bgr8=False)
            assert st.rays_primary == st.samples == size * size and st.rays_inline == 0 and st.tail_launches == 0
            frames[frame] = rgb
    seen, bad, n, skipped = {}, [], 0, 0
    for frame, x, y, want, tr in CC.spec_samples(case):
        got = frames[frame][y, x].astype(np.float64)
        if "bssrdf-coplanar" in tr:
            skipped += 1
            continue
        n += 1
        if bool((np.abs(got - want) <= 1e-4 * np.maximum(np.abs(want), 1e-3)).all()):
            for t in set(tr):
                seen[t] = seen.get(t, 0) + 1
        else:
            bad.append((frame, x, y, tr, got, want))
    print(f"shutter spec {case}: {len(bad)} of {n} samples disagree ({skipped} left out), agreeing by branch {dict(sorted(seen.items()))}")
    assert len(bad) <= 0.02 * n, f"{len(bad)} of {n} samples disagree with the float64 statement, e.g. {bad[:3]}"
    for branch, count in CC.SPEC_COUNTS[case].items():
        if branch != "left-out":
            assert seen.get(branch, 0) >= count // 2, f"only {seen.get(branch, 0)} agreeing samples went through '{branch}' ({seen})"


# ------------------------------------------------------------------------------- 4. the frames differ from the pinhole's and each other --

def test_shutter_render_counts(hip):
    hs, p, close = CC.tinyjade(64)
    frames = {}
    with hip.scene(hs) as sc:
        pin = sc.render(p)
        sc.set_shutter(*close)
        frames["shutter"] = sc.render(p)
        sc.set_lens(*SCHED_LENS)
        frames["shutter+lens"] = sc.render(p)
    for mode, (rgb, bgr, st) in frames.items():
        assert st.samples == 40 * 24 * 64 and st.rays_primary == st.samples, mode
        assert st.rays_inline == 0 and st.tail_launches == 0 and st.rays_tail == 0, mode
        assert np.isfinite(rgb).all() and rgb.max() > 0 and not same_bits(rgb, pin[0]), mode
    assert not same_bits(frames["shutter"][0], frames["shutter+lens"][0])


@pytest.mark.parametrize("env", MS.COMMON_SCHEDULES[:5] + MS.CAMERA_SCHEDULES, ids=MS.schedule_id)
def test_schedules_under_a_shutter_are_one_result(hip, monkeypatch, env):
    """Kept for its ids, which cannot all be retired in one change: tests/test_gpu_mode_seams.py runs this check for every case and environment."""
    cases = [MS.BY_NAME["shutter"], MS.BY_NAME["shutter+lens"]]
    for case, ref in zip(cases, [MS.reference(hip, c) for c in cases]):  # (the references before any environment is set)
        MS.check_schedule(hip, case, ref, env, monkeypatch.setenv)


# -------------------------------------------------------------------------------------------------------------- 5. the streak --

def _grown(m):
    W = m.shape[0]
    g = np.zeros_like(m)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            g[max(dy, 0):W + min(dy, 0), max(dx, 0):W + min(dx, 0)] |= m[max(-dy, 0):W + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return g


def test_the_streak_of_a_truck_on_the_device(hip):
    """A 0.02-wide emitter across the axis of the identity camera at depth z = 2 under a black sky, 64 x 64: a pixel is lit iff a
    sample of it hit the emitter.  The eye trucks by D = 0.5 along the camera's x over [0, 1]: at time t the emitter's centre shows at
    sample coordinate 32 - s t, s = 0.75 * 64 * D / z = 12 pixels (tests/test_shutter_cpu.py, (b)), and spans hw = 0.01 * 1.5 / z * 32 =
    0.24 pixels either way.  Pixel (x, y) is centred on sample coordinate (x, y) and a sample lies within half a pixel of that on
    each axis, so lit columns lie within [32 - s - hw - 1, 32 + hw + 1] and lit rows within those of the static render +- 1.
    Hard bounds of the geometry, not statistics.

    The spp.  Column x with 32 - s + 1 <= x <= 31 is interior: every position a sample of pixel (x, 32) can take lies, with the
    emitter's width, inside the sweep.  Such a sample hits iff its row coordinate is within hw of 32 (the jitter u2: probability
    2 hw = 0.48) and the emitter's centre at its time is within hw of its column coordinate (t uniform, the centre uniform over s
    pixels: 2 hw / s = 0.04); the two are independent: q = 0.0192 per sample.  A column stays unlit with probability (1 - q)^spp;
    at 1280 spp that is exp(1280 ln(1 - 0.0192)) = 1.7e-11, and over the 11 interior columns at most 1.9e-10 < 1e-9.  Under the
    interval [0, 0.5] the sweep is half as long and q twice as large; 5 interior columns."""
    W, z, half, D, spp = 64, 2.0, 0.01, 0.5, 1280
    s = 0.75 * W * D / z
    hw = half * 1.5 / z * W / 2
    assert s == 12.0 and hw <= 0.7
    eye = np.zeros(3, np.float32)
    eye_c, cam_c = H.camera_move(eye, CC.IDENTITY_CAM, truck=(D, 0.0, 0.0))
    assert np.array_equal(eye_c, [D, 0, 0]) and np.array_equal(cam_c[:12], CC.IDENTITY_CAM[:12])
    eye_m, cam_m = H.camera_move(eye, CC.IDENTITY_CAM, truck=(D / 2, 0.0, 0.0))
    p = B.make_params(W, W, spp, eye, CC.IDENTITY_CAM)

    def lit_of(sc, params):
        rgb, _, st = sc.render(params, want_bgr8=False)
        assert st.rays_primary == st.samples == W * W * spp
        return rgb.sum(-1) > 0

    with hip.scene(CC.emitter_on_the_axis(z, half)) as sc:
        static = lit_of(sc, p)
        static_mid = lit_of(sc, B.make_params(W, W, spp, eye_m, cam_m))
        sc.set_shutter(eye_c, cam_c)
        full = lit_of(sc, p)
        sc.set_shutter(eye_c, cam_c, 0.5, 0.5)
        instant = lit_of(sc, p)
        sc.set_shutter(eye_c, cam_c, 0.0, 0.5)
        first_half = lit_of(sc, p)
    assert static.any() and static_mid.any()
    rows = np.flatnonzero(static.any(1))
    for lit, length in ((full, s), (first_half, s / 2)):
        ys, xs = np.nonzero(lit)
        assert len(xs) and ys.min() >= rows.min() - 1 and ys.max() <= rows.max() + 1
        assert xs.min() >= 32 - length - hw - 1 and xs.max() <= 32 + hw + 1, (xs.min(), xs.max(), length)
        assert xs.min() <= 32 - length + 2, "the far end is reached within 2 pixels"
        cols = lit.any(0)
        assert cols[int(32 - length) + 1:32].all(), "an interior column is unlit"
    assert first_half.any(0).sum() < full.any(0).sum()
    assert instant.any() and not (instant & ~_grown(static_mid)).any(), "an exposure of one instant is as sharp as the static render of that pose"
    assert not (instant & static).any(), "... and 6 pixels from the open pose's"


# ------------------------------------------------------------------------------------------------------------ 6. nothing in view --

@pytest.mark.parametrize("lens", [None, (0.3, 2.0)])
def test_with_nothing_in_view_the_shutter_frame_is_the_pinhole_frame(hip, lens):
    """camera_cases.nothing_in_view: the geometry is behind the camera at both ends of the move, so that every sample of both frames is
    (10, 10, 10) bit for bit, whatever its ray."""
    eye = np.zeros(3, np.float32)
    p = B.make_params(40, 24, 8, eye, CC.IDENTITY_CAM)
    with hip.scene(CC.nothing_in_view()) as sc:
        pin = sc.render(p)
        if lens:
            sc.set_lens(*lens)
        sc.set_shutter(*H.camera_move(eye, CC.IDENTITY_CAM, truck=(0.3, 0.1, 0.0), orbit_deg=5.0))
        blur = sc.render(p)
    assert (pin[0] == 10.0).all()
    assert same_bits(blur[0], pin[0]) and np.array_equal(blur[1], pin[1])
    assert blur[2].samples == pin[2].samples == 40 * 24 * 8 and blur[2].rays_secondary == 0 and blur[2].rays_inline == 0


# ----------------------------------------------------------------------------------------------------------- 7. on top of the mode --

def test_adaptive_tiles_equal_uniform_shutter_renders(hip):
    CC.check_adaptive_tiles_equal_uniform_renders(hip, lambda sc: sc.set_shutter(*CC.tinyjade(16)[2]))


@pytest.mark.parametrize("lens", [None, CC.SPEC_LENS])
def test_guides_follow_the_shutter(hip, lens):
    hs = build("open_floor")
    S = jade_spec.Scene(hs)
    eye, cam, shutter = CC.spec_poses()
    A, f = lens if lens else (0.0, 0.0)
    size, frame = 12, 1
    p = B.make_params(size, size, 2, eye, cam, frame=frame)
    with hip.scene(hs) as sc:
        if lens:
            sc.set_lens(*lens)
        sc.set_shutter(*shutter)
        sc.render(p)
        g = sc.guides(1)
        sc.set_shutter(None)  # the render in progress keeps its shutter: so do its guides
        g_again = sc.guides(1)
        sc.render(p)
        g_off = sc.guides(1)
    with hip.scene(hs) as sc:
        if lens:
            sc.set_lens(*lens)
        sc.render(p)
        g_untouched = sc.guides(1)
    for k in g:
        assert same_bits(g[k], g_again[k]), k
        assert same_bits(g_off[k], g_untouched[k]), k
    assert not same_bits(g["depth"], g_off["depth"])
    bad = n = 0
    for y in range(size):
        for x in range(size):
            a, nrm, z = shutter_spec.guide(S, x, y, size, size, eye, cam, frame, A, f, shutter)
            want = np.concatenate([a, nrm, [z]])
            got = np.concatenate([g["albedo"][y, x], g["normal"][y, x], [g["depth"][y, x]]]).astype(np.float64)
            n += 1
            bad += not bool((np.abs(got - want) <= 1e-4 * np.maximum(np.abs(want), 1e-3)).all())
    assert bad <= 0.02 * n, f"{bad} of {n} guide samples disagree with shutter_spec.guide"


def test_denoise_under_a_shutter_is_denoise_image_on_its_own_inputs(hip):
    CC.check_denoise_is_denoise_image_on_its_own_inputs(hip, lambda sc: sc.set_shutter(*CC.tinyjade(16)[2]))


def test_cli_shutter_orbit_writes_the_python_frame(hip, tmp_path):
    size, spp = 32, 8  # the `tiny` configuration: geometry in the middle, the sky around it
    common = [CLI, "--config", "tiny", "--width", str(size), "--height", str(size), "--spp", str(spp)]
    r = subprocess.run(common + ["--shutter-orbit", "3", "--shutter-pivot", "0,0,0", "--shutter-truck", "0.05,0,0.1", "--shutter-interval", "0.25,1",
                                 "--out", "blur.pfm"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    hs, cfg = config_scene("tiny")
    p = B.params_from_config(cfg, spp=spp, walk=_abi.WALK_EARLY_EXIT)
    p.width = p.height = size
    eye_c, cam_c = H.camera_move(np.array(p.eye[:], np.float32), np.array(p.camera[:], np.float32), truck=(0.05, 0.0, 0.1), orbit_deg=3.0, pivot=(0, 0, 0))
    with hip.scene(hs) as sc:
        sc.set_shutter(eye_c, cam_c, 0.25, 1.0)
        rgb, _, _ = sc.render(p, want_bgr8=False)
        sc.set_shutter(None)
        pin, _, _ = sc.render(p, want_bgr8=False)
    assert f"shutter: closes at eye ({eye_c[0]:.9g}, {eye_c[1]:.9g}, {eye_c[2]:.9g}), exposure 0.25 .. 1 of the move" in r.stdout, r.stdout
    assert same_bits(read_pfm(tmp_path / "blur.pfm"), rgb) and not same_bits(rgb, pin)
    # the other flags keep working on top, the lens among them
    r = subprocess.run(common + ["--shutter-orbit", "2", "--aperture", "0.1", "--focus", "13.5", "--adaptive", "0.5", "--min-spp", "2", "--denoise", "--glare", "0.1",
                                 "--exposure", "auto", "--out", "all.ppm"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0 and os.path.getsize(tmp_path / "all.ppm") > 3 * size * size, r.stderr
