"""The environment lookup of the HIP module (sample_hdr, jade_shade.h) on the device, through libjade_hip_debug.so's
jade_debug_sample_hdr: bit for bit the oracle's on every direction - the undefined ones included - and within the fp32 bound of the
independent float64 statement (tests/env_spec.py) on the defined ones.  The four places a camera ray's miss calls it from (k_light_packet, k_light,
k_shade_lean, k_shade - each with its own copy of the camera ray) are reached by sky-only frames rendered through the public ABI
under JADE_LIGHT_PACKET=1, JADE_LIGHT_PACKET=0, JADE_FUSED=0 (k_shade_lean finishes every sample of such a frame) and
JADE_SHADE_SPLIT=0 (k_shade alone from the first pass on): each equals the float64 statement within the same bound, and the four are
the same bits.  tests/test_env_spec.py is the oracle's twin."""
import numpy as np
import pytest

import env_spec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=env_spec.MAP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def sky(request):
    w, h = request.param
    env = env_spec.make_map(w, h)
    return env, env_spec.sky_scene(env)


def test_device_lookup_equals_the_oracle_bits_and_the_float64_statement(hip_debug, oracle, sky):
    env, hs = sky
    h, w = env.shape[:2]
    dirs, ok = env_spec.directions(w, h)
    with oracle.scene(hs) as so:
        want = env_spec.lookup(so, "jade_oracle_sample_hdr", dirs)
    with hip_debug.scene(hs) as sd:
        got = env_spec.lookup(sd, "jade_debug_sample_hdr", dirs)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
    assert len(bad) == 0, [(dirs[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    spec = env_spec.sample_hdr(env, dirs[ok])
    err = np.abs(got[ok] - spec)
    tol = env_spec.tolerance(env)
    print(f"map {w}x{h}: worst |device - float64| {err.max():.3g}, bound {tol:.3g}")
    i = int(err.max(1).argmax())
    assert err.max() <= tol, (dirs[ok][i].tolist(), got[ok][i].tolist(), spec[i].tolist())


SCHEDULES = (("JADE_LIGHT_PACKET", "1"), ("JADE_LIGHT_PACKET", "0"), ("JADE_FUSED", "0"), ("JADE_SHADE_SPLIT", "0"))


@pytest.mark.parametrize("pose", env_spec.CAMERA_POSES, ids=lambda p: f"up{p[0]:g}_rot{p[1]:g}")
def test_sky_frames_of_every_first_pass_equal_the_float64_statement(hip, sky, pose, monkeypatch):
    env, hs = sky
    p = env_spec.sky_params(pose)
    want = env_spec.sample_hdr(env, env_spec.camera_dirs(p).reshape(-1, 3)).reshape(p.height, p.width, 3)
    tol = env_spec.tolerance(env)
    frames = []
    for key, val in SCHEDULES:
        with monkeypatch.context() as m:
            m.setenv(key, val)  # read once, at jade_scene_create
            with hip.scene(hs) as sc:
                rgb, _, st = sc.render(p)
        assert st.shaded_hits == 0 and st.rays_secondary == 0 and st.samples == p.width * p.height
        err = np.abs(rgb - want).max()
        print(f"map {env.shape[1]}x{env.shape[0]} pose {pose} {key}={val}: worst |frame - float64| {err:.3g}, bound {tol:.3g}")
        assert err <= tol, (key, val)
        frames.append(rgb)
    for (key, val), f in zip(SCHEDULES[1:], frames[1:]):
        assert np.array_equal(frames[0].view(np.uint32), f.view(np.uint32)), (key, val)


def test_sky_frame_equals_the_oracle_frame_bits(hip, oracle, sky):
    """... and the product's sky frame is the oracle's, bit for bit (one pose that sees a pole and the seam's side of the map)."""
    env, hs = sky
    p = env_spec.sky_params(env_spec.CAMERA_POSES[5])
    with oracle.scene(hs) as so:
        want, want_b, _ = so.render(p)
    with hip.scene(hs) as sc:
        got, got_b, _ = sc.render(p)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got_b, want_b)
