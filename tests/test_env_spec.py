"""The environment lookup of the oracle (sample_hdr / env_fetch, oracle/jade_oracle.c) against the independent float64 statement of
tests/env_spec.py: the v flip, the half-texel offset, mirror addressing, the poles, the seam and one-texel-wide maps - on a list of
directions and on sky-only frames - and jade_atan2f's behaviour at the seam.  tests/test_gpu_env_lookup.py asks the same of the HIP
module and that the two agree to the bit."""
import ctypes

import numpy as np
import pytest

import env_spec


@pytest.fixture(scope="module", params=env_spec.MAP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def sky(request, oracle):
    w, h = request.param
    env = env_spec.make_map(w, h)
    assert env.max() == 25 or w * h < 4
    hs = env_spec.sky_scene(env)
    with oracle.scene(hs) as sc:
        yield env, hs, sc


def test_oracle_lookup_equals_the_float64_statement(sky):
    env, hs, sc = sky
    h, w = env.shape[:2]
    dirs, ok = env_spec.directions(w, h)
    got = env_spec.lookup(sc, "jade_oracle_sample_hdr", dirs)
    want = env_spec.sample_hdr(env, dirs[ok])
    assert np.isfinite(want).all()
    err = np.abs(got[ok] - want)
    tol = env_spec.tolerance(env)
    print(f"map {w}x{h}: worst |oracle - float64| {err.max():.3g}, bound {tol:.3g}")
    i = int(err.max(1).argmax())
    assert err.max() <= tol, (dirs[ok][i].tolist(), got[ok][i].tolist(), want[i].tolist())
    assert (got[ok] <= 10).all() and (w * h < 4 or (got[ok] == 10).any())  # the clamp is reached
    # undefined directions (zero, NaN, inf): whatever comes out is a colour of the map's range, never a fault or a NaN
    assert np.isfinite(got[~ok]).all() and (got[~ok] >= 0).all() and (got[~ok] <= 10).all()


def test_oracle_poles_and_seam(sky):
    """Exactly at a pole atan2(0, 0) = 0: u = 0.5, the middle of the top / bottom row.  On the seam the sign of z picks the side:
    z = +0 reads the last column (u = 1), z = -0 the first (u = 0), as atan2f's +-pi does."""
    env, hs, sc = sky
    h, w = env.shape[:2]
    e = np.minimum(env.astype(np.float64), 10.0)
    d = np.float32([(0, 1, 0), (0, -1, 0), (-1, 0, 0.0), (-1, 0, -0.0), (-1, 0, 1e-45), (-1, 0, -1e-45)])
    got = env_spec.lookup(sc, "jade_oracle_sample_hdr", d)
    tol = env_spec.tolerance(env)
    mid = env_spec.fetch(env, np.array([0.5, 0.5]), np.array([0.0, 1.0]))
    assert np.abs(got[:2] - np.minimum(mid, 10)).max() <= tol
    vmid = np.minimum(env_spec.fetch(env, np.array([1.0, 0.0]), np.array([0.5, 0.5])), 10)
    assert np.abs(got[[2, 4]] - vmid[0]).max() <= tol and np.abs(got[[3, 5]] - vmid[1]).max() <= tol
    if h % 2 == 1:  # an odd height: v = 0.5 is a texel centre, the seam reads single texels
        assert np.abs(got[2] - e[h // 2, w - 1]).max() <= tol and np.abs(got[3] - e[h // 2, 0]).max() <= tol


@pytest.mark.parametrize("pose", env_spec.CAMERA_POSES, ids=lambda p: f"up{p[0]:g}_rot{p[1]:g}")
def test_oracle_sky_frames_equal_the_float64_statement(sky, pose):
    env, hs, sc = sky
    p = env_spec.sky_params(pose)
    rgb, _, st = sc.render(p)
    assert st.shaded_hits == 0 and st.rays_secondary == 0 and st.samples == 24 * 16
    want = env_spec.sample_hdr(env, env_spec.camera_dirs(p).reshape(-1, 3)).reshape(16, 24, 3)
    err = np.abs(rgb - want).max()
    print(f"map {env.shape[1]}x{env.shape[0]} pose {pose}: worst |oracle frame - float64| {err:.3g}, bound {env_spec.tolerance(env):.3g}")
    assert err <= env_spec.tolerance(env)


def test_atan2_at_the_seam_and_the_cases_left_as_they_are(fpm):
    """jade_atan2f(+-0, x < 0) = +-pi as atan2f and IEEE have it (it was +pi for both; PathTrace.cu:687 then reads column 0 where
    the fixed-sign version read column W - 1).  The other signed-zero / infinity cases are NOT atan2f's and stay so on purpose: no
    caller reaches them - a zero or infinite direction normalises to NaN before sample_hdr calls atan2."""
    pi = np.float32(np.pi)
    inf = np.float32(np.inf)

    def at2(y, x):
        y, x = np.float32([y]), np.float32([x])
        out = np.empty(1, np.float32)
        fpm.t_atan2(y.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), 1)
        return out[0]

    def bits(f):
        return np.float32(f).view(np.uint32)

    for x in (-1.0, -1e-45, -3.4e38, -inf):
        assert bits(at2(0.0, x)) == bits(pi) and bits(at2(-0.0, x)) == bits(-pi), x
    assert bits(at2(1e-45, -1.0)) == bits(pi) and bits(at2(-1e-45, -1.0)) == bits(-pi)
    assert bits(at2(0.0, 1.0)) == bits(0.0) and bits(at2(0.0, 0.0)) == bits(0.0)
    # kept departures from atan2f (which returns -0, +-pi, pi / 4):
    assert bits(at2(-0.0, 1.0)) == bits(0.0)
    assert bits(at2(0.0, -0.0)) == bits(0.0) and bits(at2(-0.0, -0.0)) == bits(0.0)
    assert np.isnan(at2(inf, inf))
