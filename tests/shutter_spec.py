"""The camera shutter in float64 numpy, written from the text of include/jade_bvh.h ("The shutter, stated") and NOT from the HIP code:
the ray of one sample (`ray`), the sample it starts (`sample`: the shutter ray, then tests/jade_spec.py's hit / sky / path_tracing
on the same stream, one draw further on than without a shutter) and the denoiser's guides under a shutter (`guide`).  Built on
tests/lens_spec.py as that is built on tests/jade_spec.py.

Everything is float64; only the random numbers are the fp32 values the stream defines.  A shutter is the tuple
(eye_close[3], camera_close[16], t_open, t_close); A = 0 means "no lens".  tests/test_shutter_cpu.py rests the statement on geometry
(the ends of the exposure are the two poses' own rays; a truck displaces the ray's point at depth z by t times the truck; t is uniform
on the interval) before anything is compared with it."""
import numpy as np

import jade_spec
import lens_spec

ENTRIES = (0, 1, 2, 4, 5, 6, 8, 9, 10)  # the nine entries of the matrix jade_transform(v, 0, .) multiplies by v


def time_of(ut, t_open, t_close):
    return t_open + ut * (t_close - t_open)


def pose_at(t, eye, cam, eye_close, cam_close):
    """(eye_t, cam_t): eye and the nine entries interpolated one by one, every other entry of cam_t is cam's.  t: scalar or [n]."""
    t = np.asarray(t, np.float64)
    eye, cam, eye_close, cam_close = (np.asarray(v, np.float64) for v in (eye, cam, eye_close, cam_close))
    eye_t = eye + t[..., None] * (eye_close - eye)
    cam_t = np.broadcast_to(cam, t.shape + (16,)).copy()
    for j in ENTRIES:
        cam_t[..., j] = cam[..., j] + t * (cam_close[..., j] - cam[..., j])
    return eye_t, cam_t


def ray(x, y, W, H, eye, cam, A, f, shutter, u1, u2, u3, u4, ut):
    """(origin, dir) of the shutter ray.  Scalars, or arrays of rows (eye [..., 3], cam [..., 16], and the shutter's members alike).
    Where A == 0 the ray is the pinhole's of the pose at t and u3, u4 are not read; where A > 0 it is lens_spec.ray of that pose."""
    eye_close, cam_close, t_open, t_close = shutter
    t = time_of(np.asarray(ut, np.float64), np.asarray(t_open, np.float64), np.asarray(t_close, np.float64))
    eye_t, cam_t = pose_at(t, eye, cam, eye_close, cam_close)
    A = np.asarray(A, np.float64)
    o_p, d_p = lens_spec.pinhole_ray(x, y, W, H, eye_t, cam_t, u1, u2)
    if not (A > 0).any():
        return np.broadcast_to(o_p, d_p.shape).copy(), d_p
    f_safe = np.where(A > 0, np.asarray(f, np.float64), 1.0)  # (f is not read without a lens)
    o_l, d_l = lens_spec.ray(x, y, W, H, eye_t, cam_t, A, f_safe, u1, u2, u3, u4)
    lens = (A > 0)[..., None]
    return np.where(lens, o_l, o_p), np.where(lens, d_l, d_p)


def draws(rng, A):
    """u1, u2, (u3, u4 under a lens, else 0, 0), ut - in the order of the statement."""
    u1, u2 = next(rng), next(rng)
    u3, u4 = (next(rng), next(rng)) if A > 0 else (0.0, 0.0)
    return u1, u2, u3, u4, next(rng)


def sample(S, x, y, width, height, eye, cam, frame, A, f, shutter, trace=None):
    """One sample of pixel (x, y) under the shutter: three or five draws for the ray, then jade_spec's pixel assembly on the same stream."""
    rng = jade_spec.wang_stream(x, y, frame)
    trace = trace if trace is not None else []
    o, d = ray(x, y, width, height, eye, cam, A, f, shutter, *draws(rng, A))
    h, hp = S.hit(o, d, -1)
    if h < 0:
        trace.append("sky")
        return S.sky(d)
    return S.emis[h] + jade_spec.path_tracing(S, rng, h, hp, -d, trace)


def guide(S, x, y, width, height, eye, cam, frame, A, f, shutter):
    """Guide sample 0 of pixel (x, y) under the shutter, for scenes WITHOUT mirrors: (albedo[3], normal[3], depth) as lens_spec.guide."""
    rng = jade_spec.wang_stream(x, y, frame)
    o, d = ray(x, y, width, height, eye, cam, A, f, shutter, *draws(rng, A))
    h, hp = S.hit(o, d, -1)
    if h < 0:
        return np.ones(3), np.zeros(3), 0.0
    assert S.reflex[h] == 0, "shutter_spec.guide does not follow mirrors"
    n = S.norm[h]
    if n @ d > 0:
        n = -n
    return S.brdf[h].copy(), n.copy(), float((hp - o) @ d)
