"""The thin-lens camera in float64 numpy, written from the text of include/jade_bvh.h ("The lens, stated") and NOT from the HIP
code: the ray of one sample (`ray`), the sample it starts (`sample`: the lens ray, then tests/jade_spec.py's hit / sky /
path_tracing on the same stream, two draws further on than the pinhole's) and the denoiser's guides under a lens (`guide`).

Everything is float64; only the random numbers are the fp32 values the stream defines.  tests/test_lens_cpu.py rests the statement on
geometry (every lens ray of a jitter meets the pinhole ray in the plane of focus; the circle of confusion's closed form; a uniform
disk) before anything is compared with it."""
import numpy as np

import jade_spec

PI = jade_spec.PI  # 3.1415926 as everywhere


def offsets(x, y, W, H, u1, u2):
    """left_offset, up_offset of pixel (x, y) with jitter (u1, u2): the pinhole's statements (PathTrace.cu:1428-1434)."""
    left = (-1 + 2.0 / W * (x + u1 - 0.5)) * (W / H)
    up = -1 + 2.0 / H * (y + u2 - 0.5)
    return left, up


def transform(v, cam):
    """jade_transform(v, 0, cam) with cam[4 * col + row]: v [..., 3], cam [..., 16] -> [..., 3]."""
    M = np.asarray(cam, np.float64)
    v = np.asarray(v, np.float64)
    return np.stack([sum(M[..., 4 * c + r] * v[..., c] for c in range(3)) for r in range(3)], axis=-1)


def lens_point(A, u3, u4):
    r = A * np.sqrt(u3)
    phi = float(np.float32(2 * PI)) * u4  # fl(2 PI): the one float32 constant of the statement
    return r * np.cos(phi), r * np.sin(phi)


def ray(x, y, W, H, eye, cam, A, f, u1, u2, u3, u4):
    """(origin, dir) of the lens ray; A = aperture_radius, f = focus_distance.  Scalars, or arrays of rows (eye [..., 3], cam [..., 16])."""
    x, y, W, H, A, f, u1, u2, u3, u4 = (np.asarray(v, np.float64) for v in (x, y, W, H, A, f, u1, u2, u3, u4))
    left, up = offsets(x, y, W, H, u1, u2)
    lx, ly = lens_point(A, u3, u4)
    k = f / 1.5
    d_c = np.stack(np.broadcast_arrays(left * k - lx, up * k - ly, -1.5 * k), axis=-1)
    d = transform(d_c, cam)
    d = d / np.sqrt((d * d).sum(-1))[..., None]
    o = np.asarray(eye, np.float64) + transform(np.stack(np.broadcast_arrays(lx, ly, np.zeros_like(lx)), axis=-1), cam)
    return o, d


def pinhole_ray(x, y, W, H, eye, cam, u1, u2):
    x, y, W, H, u1, u2 = (np.asarray(v, np.float64) for v in (x, y, W, H, u1, u2))
    left, up = offsets(x, y, W, H, u1, u2)
    d = transform(np.stack(np.broadcast_arrays(left, up, np.full_like(left, -1.5)), axis=-1), cam)
    return np.asarray(eye, np.float64), d / np.sqrt((d * d).sum(-1))[..., None]


def sample(S, x, y, width, height, eye, cam, frame, A, f, trace=None):
    """One sample of pixel (x, y) under the lens: four draws for the ray, then jade_spec's pixel assembly on the same stream."""
    rng = jade_spec.wang_stream(x, y, frame)
    trace = trace if trace is not None else []
    u1, u2, u3, u4 = next(rng), next(rng), next(rng), next(rng)
    o, d = ray(x, y, width, height, eye, cam, A, f, u1, u2, u3, u4)
    h, hp = S.hit(o, d, -1)
    if h < 0:
        trace.append("sky")
        return S.sky(d)
    return S.emis[h] + jade_spec.path_tracing(S, rng, h, hp, -d, trace)


def guide(S, x, y, width, height, eye, cam, frame, A, f):
    """Guide sample 0 of pixel (x, y) under the lens, for scenes WITHOUT mirrors (include/jade_bvh.h, the guide statement with t = 1 and
    no continuation): (albedo[3], normal[3], depth).  A miss: albedo 1, normal 0, depth 0."""
    rng = jade_spec.wang_stream(x, y, frame)
    u1, u2, u3, u4 = next(rng), next(rng), next(rng), next(rng)
    o, d = ray(x, y, width, height, eye, cam, A, f, u1, u2, u3, u4)
    h, hp = S.hit(o, d, -1)
    if h < 0:
        return np.ones(3), np.zeros(3), 0.0
    assert S.reflex[h] == 0, "lens_spec.guide does not follow mirrors"
    n = S.norm[h]
    if n @ d > 0:
        n = -n
    return S.brdf[h].copy(), n.copy(), float((hp - o) @ d)
